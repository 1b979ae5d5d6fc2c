#!/usr/bin/env python3
"""The block-local codecs' layer launch under hipGraph capture: ONE launch per layer on a private gate slot (cfx_set_captured_layer) against
the capturable sequence compress ; reconstruct and against the eager one-launch step, in ONE process on one MI355X (developer tool; output
committed as profiles/captured_layer_rows.json).

  workload   the FLUX shard (544, 3072): K,V + 14 looped-back peers per layer, 57 layers of distinct state; a step = the 57 layer calls
  codecs     MXINT8 bf16, BINARY_BLOCK 64 fp16, MXFP4
  steps      ms per step, per codec, of three forms measured in the same process, their groups interleaved (eager, sequence, one-launch,
             eager, ...): the EAGER one-launch step (57 host calls a step on a stream), the CAPTURED SEQUENCE step (a graph of the 57
             calls captured without a pool: 114 kernel nodes) and the CAPTURED ONE-LAUNCH step (the same capture with a pool: 57 kernel
             nodes).  Every figure: device events around a group of `--steps` steps, `--groups` groups; the median of the groups and
             their spread (max - min).  `wins`: the one-launch median is below the sequence median by more than 3 x the larger spread
  kernels    us per layer of the captured layer kernel k_*_layer_cap against its eager twin k_*_layer, from a rocprofv3 --kernel-trace of
             `--trace-run` (a run of its own: tracing slows the host), reduced by tools/trace_kernel_avg.py and merged with
             `--merge-kernels`: what the 64-bit arrivals and the entry tickets cost

usage: python tools/captured_layer_rows.py [--out profiles/captured_layer_rows.json] [--groups 5] [--steps 50]
       rocprofv3 --kernel-trace --output-format csv -d DIR -o cap -- python tools/captured_layer_rows.py --trace-run
       python tools/trace_kernel_avg.py DIR/.../cap_kernel_trace.csv kernels.json
       python tools/captured_layer_rows.py --merge-kernels kernels.json [--out ...]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")          # (before torch initialises HIP, as tools/config_table.py does)

N, C, L, NP = 544, 3072, 57, 14
ROWS = [("MXINT8 bf16", 0x110, 0, "k_mxi8_layer"), ("BINARY_BLOCK 64 fp16", 10, 64, "k_bb_layer"), ("MXFP4 fp16", 8, 0, "k_mx_layer")]


class Workload:
    def __init__(self, cabi, param):
        import torch
        from compactfusion_amd import _lib, codecs as K
        self.torch, self.lib, self.ctx = torch, _lib.load(), K.context(0)
        self.cabi, self.param = cabi, param
        dt = torch.bfloat16 if cabi & 0x100 else torch.float16
        g = torch.Generator(device="cuda").manual_seed(1)
        self.own = torch.randn(L, 2, N, C, generator=g, device="cuda").to(dt)
        self.xs = (self.own.float() + 0.1 * torch.randn(L, 2, N, C, generator=g, device="cuda")).to(dt)
        self.peer = torch.randn(L, NP, N, C, generator=g, device="cuda").to(dt)
        nbytes = K.packet_bytes(cabi, N, C, param)
        self.pk = torch.zeros(L, 2, (nbytes + 255) // 256 * 256, dtype=torch.uint8, device="cuda")
        xs, own, pk, peer = self.xs, self.own, self.pk, self.peer
        self.comp = [(_lib.CompItem * 2)(*[_lib.CompItem(xs[l, b].data_ptr(), own[l, b].data_ptr(), own[l, b].data_ptr(), pk[l, b].data_ptr())
                                           for b in range(2)]) for l in range(L)]
        self.gated = [(_lib.DecompItem * NP)(*[_lib.DecompItem(pk[l, j % 2].data_ptr(), peer[l, j].data_ptr(), peer[l, j].data_ptr())
                                               for j in range(NP)]) for l in range(L)]
        self.flags = _lib.FLAG_UPDATE_CACHE
        self.stream = torch.cuda.Stream()

    def step(self, sh):
        lib, ctx = self.lib, self.ctx
        for l in range(L):
            rc = lib.cfx_compress_batch_gated(ctx, self.cabi, N, C, self.param, self.flags, 2, self.comp[l], 0, None, NP, self.gated[l], None, 0, sh)
            assert rc == 0, lib.cfx_last_error_string(ctx)

    def capture(self, pool):
        """a graph of one step, captured with a pool of `pool` slots; (graph, capture-time calls that took one launch, ... the sequence)"""
        torch, lib, ctx = self.torch, self.lib, self.ctx
        from compactfusion_amd import codecs as K
        assert lib.cfx_set_captured_layer(ctx, pool) == 0, lib.cfx_last_error_string(ctx)
        s0 = K.captured_layer_stats(0)
        self.stream.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(self.stream):
            with torch.cuda.graph(graph, stream=self.stream):
                self.step(self.stream.cuda_stream)
        torch.cuda.synchronize()
        s1 = K.captured_layer_stats(0)
        return graph, s1["one_launch"] - s0["one_launch"], s1["sequence"] - s0["sequence"]

    def timed(self, fn, steps):
        """ms per step of `steps` runs of fn on the workload's stream (device events around the group)"""
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            a.record(self.stream)
            for _ in range(steps):
                fn()
            b.record(self.stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps

    def forms(self):
        """the three forms of a step as callables on the workload's stream; the graphs stay alive in the returned dict"""
        lib, ctx = self.lib, self.ctx
        g_seq, one, seq = self.capture(0)
        assert (one, seq) == (0, L), (one, seq)
        g_one, one, seq = self.capture(64)
        assert (one, seq) == (L, 0), (one, seq)
        sh = self.stream.cuda_stream
        return {"eager_one_launch": lambda: self.step(sh), "captured_sequence": g_seq.replay, "captured_one_launch": g_one.replay,
                "_keep": (g_seq, g_one)}

    def release(self, forms):
        forms.clear()
        self.torch.cuda.synchronize()
        assert self.lib.cfx_captured_layer_release(self.ctx) == 0 and self.lib.cfx_set_captured_layer(self.ctx, 0) == 0
        assert self.lib.cfx_gate_errors(self.ctx) == 0


def measure(groups, steps):
    import torch
    res = {}
    for name, cabi, param, _ in ROWS:
        w = Workload(cabi, param)
        forms = w.forms()
        names = [k for k in forms if not k.startswith("_")]
        for k in names:                                   # warm-up: every form, its code objects and the graph's first launch
            w.timed(forms[k], 5)
        runs = {k: [] for k in names}
        for g in range(groups):
            for k in (names if g % 2 == 0 else names[::-1]):
                runs[k].append(round(w.timed(forms[k], steps), 5))
        row = {k: {"groups_ms": runs[k], "median_ms": round(statistics.median(runs[k]), 5), "spread_ms": round(max(runs[k]) - min(runs[k]), 5)}
               for k in names}
        gain = row["captured_sequence"]["median_ms"] - row["captured_one_launch"]["median_ms"]
        bar = 3 * max(row["captured_sequence"]["spread_ms"], row["captured_one_launch"]["spread_ms"])
        row["one_launch_minus_sequence_ms"] = round(-gain, 5)
        row["bar_3x_spread_ms"] = round(bar, 5)
        row["wins"] = bool(gain > bar)
        res[name] = row
        print(name, json.dumps(row), flush=True)
        w.release(forms)
        del w
        torch.cuda.empty_cache()
    return res


def trace_run():
    """what the kernel trace is taken of: per codec 3 eager steps and 3 replays of the one-launch graph after a warm-up of each"""
    import torch
    for name, cabi, param, _ in ROWS:
        w = Workload(cabi, param)
        forms = w.forms()
        for k in ("eager_one_launch", "captured_one_launch"):
            w.timed(forms[k], 4)
        w.release(forms)
        del w
        torch.cuda.empty_cache()
    print("trace run done", flush=True)


def merge_kernels(path, out):
    with open(path) as f:
        ks = json.load(f)["kernels"]
    with open(out) as f:
        res = json.load(f)
    rows = {}
    for name, _, _, kern in ROWS:
        eager = {k: v for k, v in ks.items() if k.split("<")[0] == kern}
        cap = {k: v for k, v in ks.items() if k.split("<")[0] == kern + "_cap"}
        assert len(eager) == 1 and len(cap) == 1, (name, sorted(ks))
        (en, e), (cn, c) = list(eager.items())[0], list(cap.items())[0]
        rows[name] = {"eager_kernel": en, "captured_kernel": cn,
                      "eager_us": {k: e[k] for k in ("launches", "median_us", "avg_us", "min_us", "max_us")},
                      "captured_us": {k: c[k] for k in ("launches", "median_us", "avg_us", "min_us", "max_us")},
                      "captured_minus_eager_median_us": round(c["median_us"] - e["median_us"], 3)}
    res["kernels"] = {"source": "rocprofv3 --kernel-trace of `tools/captured_layer_rows.py --trace-run`, tools/trace_kernel_avg.py", "rows": rows}
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res["kernels"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "captured_layer_rows.json"))
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge-kernels")
    args = ap.parse_args()
    if args.merge_kernels:
        return merge_kernels(args.merge_kernels, args.out)
    if args.trace_run:
        return trace_run()
    assert args.groups >= 5 and args.steps >= 50, "at least 5 groups of at least 50 steps"
    import torch
    res = {"unit": __doc__.split("\n\n")[1], "device": torch.cuda.get_device_name(0), "shape": [N, C], "layers": L, "peers": NP,
           "groups": args.groups, "steps_per_group": args.steps, "steps": measure(args.groups, args.steps)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
