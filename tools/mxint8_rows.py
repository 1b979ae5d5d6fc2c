#!/usr/bin/env python3
"""The block-scaled 8-bit codec (MXINT8, codec 16) beside INT8, MXFP4 and the 1-bit codec at the FLUX shard, and beside INT8 / INT4 at the
small-shard BASELINE configurations 1 and 2, in ONE process on one MI355X (developer tool; output committed as
profiles/mxint8_config_rows.json).

  layer_launch  us of the codec launches one cfx_compress_batch_gated call makes (cfx_profile_read: events on the dispatch; the block-local
                codecs and the 1-bit codec: kernel id 31 alone; INT8: whatever ids its call launches, summed per call and listed), K,V +
                14 looped-back peers of (544, 3072), 20 distinct layers of state, 100 calls after 20 warm-up calls; two rounds over the rows
  steps         ms per step of tools/config_table.py gpu_step (one exchange-layer op per layer), repetitions interleaved over the rows: the
                FLUX shard (544, 3072) x 57, config 1's tensor (4096, 1152) x 1 and config 2's shard (1024, 1152) x 28
  copy_probe    TB/s (read + write) of cfx_copy_probe on 96 MiB, before, between and after: what the fractions are of
  quality_g12   relative reconstruction error per step of K (seed 4242) and V (4243) on the G12 drift inputs, residual 1 with error feedback,
                from the GPU path (codecs.compress on the device, states read back)

usage: python tools/mxint8_rows.py [--out profiles/mxint8_config_rows.json] [--reps 3]
       python tools/mxint8_rows.py --launch-only      the layer launch of the MXINT8 and MXFP4 rows alone, two rounds, printed: one process
                                                      of an A/B of two builds (CFX_LIBCFX_PATH picks the library; profiles: "in_flight_ab")"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import config_table as CT          # noqa: E402  (sets GPU_MAX_HW_QUEUES before torch initialises HIP)
import torch                       # noqa: E402

from compactfusion_amd import _lib, codecs as K      # noqa: E402

N, C, L, NP, LAYERS = 544, 3072, 57, 14, 20
KID_LAYER = 31
ROWS = [("BINARY fp16", 1, 0), ("INT8 fp16", 4, 0), ("MXFP4 fp16", 8, 0), ("MXINT8 fp16", 16, 0), ("MXINT8 bf16", 0x110, 0)]
# (name, codec argument, param, (N, C), layers, tensors compressed, tensors reconstructed, update on compress): tools/config_table.py's rows
SMALL = [("config 1 tensor (4096, 1152), world 1: INT8", 4, 0, (4096, 1152), 1, 1, 1, True),
         ("config 1 tensor (4096, 1152), world 1: MXINT8", 16, 0, (4096, 1152), 1, 1, 1, True),
         ("config 2 shard (1024, 1152) x 28: INT4", 3, 0, (1024, 1152), 28, 2, 4, False),
         ("config 2 shard (1024, 1152) x 28: INT8", 4, 0, (1024, 1152), 28, 2, 4, False),
         ("config 2 shard (1024, 1152) x 28: MXINT8", 16, 0, (1024, 1152), 28, 2, 4, False)]


def layer_launch(cabi, param):
    lib, ctx = _lib.load(), K.context(0)
    dt = torch.bfloat16 if cabi & 0x100 else torch.float16
    g = torch.Generator(device="cuda").manual_seed(1)
    own = torch.randn(LAYERS, 2, N, C, generator=g, device="cuda").to(dt)
    xs = (own.float() + 0.1 * torch.randn(LAYERS, 2, N, C, generator=g, device="cuda")).to(dt)
    peer = torch.randn(LAYERS, NP, N, C, generator=g, device="cuda").to(dt)
    nbytes = K.packet_bytes(cabi, N, C, param)
    pk = torch.zeros(LAYERS, 2, (nbytes + 255) // 256 * 256, dtype=torch.uint8, device="cuda")
    wsb = lib.cfx_workspace_bytes(cabi, N, C, param, 2)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    comp = [(_lib.CompItem * 2)(*[_lib.CompItem(xs[l, b].data_ptr(), own[l, b].data_ptr(), own[l, b].data_ptr(), pk[l, b].data_ptr())
                                  for b in range(2)]) for l in range(LAYERS)]
    gated = [(_lib.DecompItem * NP)(*[_lib.DecompItem(pk[l, j % 2].data_ptr(), peer[l, j].data_ptr(), peer[l, j].data_ptr())
                                      for j in range(NP)]) for l in range(LAYERS)]
    stream = torch.cuda.Stream()

    def run(n):
        for i in range(n):
            l = i % LAYERS
            rc = lib.cfx_compress_batch_gated(ctx, cabi, N, C, param, _lib.FLAG_UPDATE_CACHE, 2, comp[l], 0, None, NP, gated[l],
                                              ws.data_ptr() if wsb else None, wsb, stream.cuda_stream)
            assert rc == 0, lib.cfx_last_error_string(ctx)
    torch.cuda.synchronize()
    run(20)
    torch.cuda.synchronize()
    assert lib.cfx_profile_enable(ctx, 1024, 0xffffffff, 1) == 0
    run(100)
    torch.cuda.synchronize()
    ids, ms = (ctypes.c_int * 1024)(), (ctypes.c_float * 1024)()
    n = lib.cfx_profile_read(ctx, ids, ms, 1024)
    lib.cfx_profile_enable(ctx, 0, 0, 1)
    assert lib.cfx_gate_errors(ctx) == 0
    c, d = CT.alg_pair(cabi, param)
    k = n // 100                                            # launches a call makes; their kernel ids, the same for every call
    per_call = [ids[i] for i in range(k)]
    if n == 0 or n % 100 or any([ids[q * k + j] for j in range(k)] != per_call for q in range(100)):
        # calls that differ in what they launch (no block-local codec does): the mean per call alone
        assert (cabi & 0xff) == 4, ("not the one-launch layer form", sorted({ids[i] for i in range(n)}))
        return {"mean_us": round(sum(ms[i] for i in range(n)) * 1e3 / 100, 2), "kernel_ids": sorted({ids[i] for i in range(n)}),
                "alg_bytes": int(N * C * (2 * c + NP * d)), "packet_bytes": nbytes}
    if (cabi & 0xff) != 4:
        assert per_call == [KID_LAYER], ("not the one-launch layer form", per_call)
    us = [sum(ms[q * k + j] for j in range(k)) * 1e3 for q in range(100)]
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "kernel_ids": per_call,
            "alg_bytes": int(N * C * (2 * c + NP * d)), "packet_bytes": nbytes}


def copy_probe():
    lib, ctx = _lib.load(), K.context(0)
    nb = 96 << 20
    src = [torch.empty(nb, dtype=torch.uint8, device="cuda").fill_(i) for i in range(4)]
    dst = [torch.empty(nb, dtype=torch.uint8, device="cuda") for _ in range(4)]
    st = torch.cuda.Stream()
    best = 0.0
    for rep in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            a.record(st)
            for i in range(8):
                assert lib.cfx_copy_probe(ctx, dst[i % 4].data_ptr(), src[i % 4].data_ptr(), nb, st.cuda_stream) == 0
            b.record(st)
        torch.cuda.synchronize()
        if rep:
            best = max(best, 8 * 2 * nb / (a.elapsed_time(b) * 1e-3) / 1e12)
    return round(best, 3)


def quality_g12(cid, param):
    spec = importlib.util.spec_from_file_location("make_golden_quality", os.path.join(REPO, "tests", "golden", "make_golden_quality.py"))
    mq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mq)
    out = {}
    for name, seed in (("K", 4242), ("V", 4243)):
        xs = mq.drift(seed, 28)
        state = xs[0].cuda().clone()
        errs = []
        for x in xs[1:]:
            xd = x.cuda()
            _, state = K.compress(cid, xd, state, mq.N, mq.C, param, update_cache=True)
            errs.append(float((state.double() - xd.double()).norm() / xd.double().norm()))
        out[name] = {"mean": round(statistics.mean(errs), 5), "max": round(max(errs), 5), "per_step": [round(e, 5) for e in errs]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mxint8_config_rows.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launch-only", action="store_true")
    args = ap.parse_args()
    if args.launch_only:
        rows = [r for r in ROWS if r[0].startswith(("MXINT8", "MXFP4"))]
        out = {n: [] for n, _, _ in rows}
        for rnd in range(2):
            for name, cabi, param in rows:
                out[name].append(layer_launch(cabi, param))
                torch.cuda.empty_cache()
        print(json.dumps({"library": os.environ.get("CFX_LIBCFX_PATH") or "as built", "rows": out}, indent=1))
        return
    res = {"unit": __doc__.split("\n\n")[1], "device": torch.cuda.get_device_name(0), "layer_launch": {n: [] for n, _, _ in ROWS},
           "steps": {}, "copy_probe": {}}
    res["copy_probe"]["first_TBps"] = copy_probe()
    for rnd in range(2):
        for name, cabi, param in (ROWS if rnd == 0 else ROWS[::-1]):
            res["layer_launch"][name].append(layer_launch(cabi, param))
            torch.cuda.empty_cache()
            print(name, res["layer_launch"][name][-1], flush=True)
    res["copy_probe"]["after_layers_TBps"] = copy_probe()
    steps = [("FLUX shard: " + n, cabi, param, (N, C), L, 2, NP, True) for n, cabi, param in ROWS] + SMALL
    runs = {s[0]: [] for s in steps}
    for rep in range(args.reps):
        for name, cabi, param, (n_, c_), layers, ncomp, nrec, upd in (steps if rep % 2 == 0 else steps[::-1]):
            runs[name].append(round(CT.gpu_step(cabi, param, n_, c_, layers, ncomp, nrec, upd), 4))
            torch.cuda.empty_cache()
            print(name, runs[name][-1], "ms/step", flush=True)
    for name, cabi, param, (n_, c_), layers, ncomp, nrec, upd in steps:
        res["steps"][name] = {"alg_bytes": CT.alg_bytes(cabi, n_, c_, layers, ncomp, nrec, upd, param), "runs": runs[name],
                              "median": statistics.median(runs[name])}
    res["copy_probe"]["end_TBps"] = copy_probe()
    res["quality_g12"] = {"what": "relative reconstruction error of the error-feedback state per step on the G12 drift inputs ((128, 3072), 28 "
                                  "steps, step 0 WARMUP; tests/golden/make_golden_quality.py), from the GPU path (codecs.compress)"}
    for name, cid, param in (("INT8", 4, 0), ("MXFP4", 8, 0), ("MXINT8", 16, 0)):
        res["quality_g12"][name] = quality_g12(cid, param)
        print(name, {k: (v["mean"], v["max"]) for k, v in res["quality_g12"][name].items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
