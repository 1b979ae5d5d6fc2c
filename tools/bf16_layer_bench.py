"""The FLUX exchange step of bench.py's headline, in fp16 and in bf16, in ONE process: 57 layers x {K, V} of (544, 3072), 1-bit residual
codec with error feedback, 8 logical ranks looped back, one layer call per layer (cfx_compress_batch_gated: 2 compress items, 14 gated
reconstruction items, the own error-feedback update inside the launch).  The bytes moved are the same for both element types; the fp16
step IS the code every earlier measurement ran.

Protocol: every shape warmed up first; repetitions of the two element types ALTERNATE (fp16, bf16, fp16, ...), each repetition `--steps`
steps between two device events on the launch stream, ended by a synchronise; median and spread (min .. max) per element type.  The
allowance for the comparison is the measured spread of the fp16 repetitions themselves.  Prints one JSON line; --out writes it to a file.

usage: python tools/bf16_layer_bench.py [--reps 7] [--steps 50] [--warmup 5] [--out profiles/bf16_layer_step.json]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")

L, N, C, W = 57, 544, 3072, 8
CODEC = 1


class Step:
    """The states, inputs and packet slots of the 57 layers in one element type, and the layer calls bound to them."""

    def __init__(self, dtype, seed):
        import torch
        from compactfusion_amd import _lib, codecs as K
        self.torch, self._lib, self.lib, self.ctx = torch, _lib, _lib.load(), K.context(0)
        self.cabi = K.codec_arg(CODEC, dtype)
        g = torch.Generator(device="cuda").manual_seed(seed)
        x0 = torch.randn(L, 2, N, C, generator=g, device="cuda")
        self.xs = [(x0 + 0.1 * (s + 1) * torch.randn(L, 2, N, C, generator=g, device="cuda")).to(dtype) for s in range(2)]
        self.own = x0.to(dtype)
        self.peer = self.own.unsqueeze(1).repeat(1, W - 1, 1, 1, 1).contiguous()
        self.slot = (K.packet_bytes(self.cabi, N, C) + 255) // 256 * 256
        self.pk = torch.zeros(L, 2, self.slot, dtype=torch.uint8, device="cuda")
        self.wsb = self.lib.cfx_workspace_bytes(self.cabi, N, C, 0, 2)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.comp = [[(_lib.CompItem * 2)(*[_lib.CompItem(self.xs[s][l, b].data_ptr(), self.own[l, b].data_ptr(), self.own[l, b].data_ptr(),
                                                          self.pk[l, b].data_ptr()) for b in range(2)]) for l in range(L)] for s in range(2)]
        self.gated = [(_lib.DecompItem * (2 * (W - 1)))(*[_lib.DecompItem(self.pk[l, b].data_ptr(), self.peer[l, p, b].data_ptr(), self.peer[l, p, b].data_ptr())
                                                          for p in range(W - 1) for b in range(2)]) for l in range(L)]
        self.n = 0

    def run(self, steps, sh):
        lib, ctx, fn = self.lib, self.ctx, self.lib.cfx_compress_batch_gated
        wsp, ng = self.ws.data_ptr(), 2 * (W - 1)
        for _ in range(steps):
            comp = self.comp[self.n & 1]
            self.n += 1
            for l in range(L):
                rc = fn(ctx, self.cabi, N, C, 0, self._lib.FLAG_UPDATE_CACHE, 2, comp[l], 0, None, ng, self.gated[l], wsp, self.wsb, sh)
                if rc != 0:
                    raise RuntimeError("layer call failed: " + (lib.cfx_last_error_string(ctx) or b"").decode())

    def timed(self, steps, stream):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            self.run(steps, stream.cuda_stream)
            b.record(stream)
        torch.cuda.synchronize()
        if self.lib.cfx_gate_errors(self.ctx) != 0:
            raise RuntimeError("an in-launch wait timed out during the timed window")
        return a.elapsed_time(b) / steps            # ms per step


def kernels_per_layer(step, stream):
    """the library's per-launch hooks: which kernels one layer call launches"""
    import ctypes
    lib, ctx = step.lib, step.ctx
    lib.cfx_profile_enable(ctx, 8 * L, 0xffffffff, 1)
    step.run(1, stream.cuda_stream)
    step.torch.cuda.synchronize()
    ids, ms = (ctypes.c_int * (8 * L))(), (ctypes.c_float * (8 * L))()
    n = lib.cfx_profile_read(ctx, ids, ms, 8 * L)
    lib.cfx_profile_enable(ctx, 0, 0, 1)
    return n / L, sorted({(lib.cfx_kernel_name(ids[i]) or b"").decode() for i in range(n)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 repetitions per element type")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bf16_layer_bench.py measures on the GPU: none found")
    stream = torch.cuda.Stream()
    forms = {"fp16": Step(torch.float16, 1), "bf16": Step(torch.bfloat16, 1)}
    launches = {}
    for name, st in forms.items():
        with torch.cuda.stream(stream):
            st.run(args.warmup, stream.cuda_stream)
        torch.cuda.synchronize()
        launches[name] = kernels_per_layer(st, stream)
    times = {"fp16": [], "bf16": []}
    for rep in range(args.reps):
        for name in (("fp16", "bf16") if rep % 2 == 0 else ("bf16", "fp16")):       # alternating, and alternating who goes first
            times[name].append(forms[name].timed(args.steps, stream))
    res = {"workload": f"FLUX exchange step: {L} layers x K,V ({N}, {C}), 1-bit + error feedback, {W} logical ranks looped back, one layer call per layer",
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "steps_per_rep": args.steps, "warmup_steps": args.warmup, "unit": "ms per step"}
    for name, t in times.items():
        res[name] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4),
                     "spread": round(max(t) - min(t), 4), "all": [round(v, 4) for v in t],
                     "launches_per_layer": launches[name][0], "kernels": launches[name][1]}
    lo, hi = res["fp16"]["min"], res["fp16"]["max"]
    res["bf16_over_fp16_median"] = round(res["bf16"]["median"] / res["fp16"]["median"], 4)
    res["allowance"] = "the spread of the fp16 repetitions: [%.4f, %.4f] ms" % (lo, hi)
    res["bf16_median_within_fp16_spread"] = bool(lo <= res["bf16"]["median"] <= hi)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
