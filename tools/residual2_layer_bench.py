#!/usr/bin/env python3
"""A denoise step with second-order residuals (CompactConfig(residual=2)) through the plugin API, against the same step of another tree.

Workload: the FLUX shard (544, 3072), 57 layers, 8 logical ranks looped back on one GPU; BINARY and INT2 with residual 2 through
`compact_fwd` (ring gather schedule, lane off, attention replaced by a no-op - as tools/plugin_config_bench.py does), and the residual-1
step of the same codec beside it.  Only API that both trees have: the same file runs on a checkout of the parent commit.

  python tools/residual2_layer_bench.py --run BINARY 2 [--tree DIR]      one run, one process: prints {"ms_per_step": ...}
  python tools/residual2_layer_bench.py --parent DIR [--this DIR] [--parent-commit H --this-commit H] [--json profiles/residual2_layer_step.json]
      the protocol: 3 repeats; in every repeat the parent tree first, then this tree; one process per run; 20 steps after the warm-up
      (2 WARMUP steps + 3 compressed ones); medians with min .. max over the repeats."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--run", nargs=2, metavar=("CODEC", "RESIDUAL"))
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--parent")
ap.add_argument("--this", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--parent-commit", default="")
ap.add_argument("--this-commit", default="")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--json", default=None)
args = ap.parse_args()

W, L, N, H, D = 8, 57, 544, 24, 128


def one_run(codec, residual):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    sys.path.insert(0, args.tree)
    import torch
    import compactfusion_amd
    from compactfusion_amd import _lib, codecs as K
    from compactfusion_amd.compact import ring, main as cm, xlayer
    compactfusion_amd.configure(lane="off")
    from compactfusion_amd.compact.utils import CompactConfig, COMPACT_COMPRESS_TYPE as T
    from compactfusion_amd.collector import collector
    from compactfusion_amd.prof import Profiler
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib, ctx = _lib.load(), K.context(0)
    Profiler.instance().disable()
    collector.init(collector.Collector("/tmp/none", enabled=False))
    ring.dist.get_rank = lambda g=None: 0
    ring.dist.get_world_size = lambda g=None: W
    ring.dist.all_gather_into_tensor = lambda recv, send, group=None: recv.view(W, -1).copy_(send.view(1, -1).expand(W, -1))
    xlayer.set_p2p_loopback(True)
    CT, warm = T[codec], 2 if residual == 2 else 1
    kw = dict(residual=2, ef=True, comp_rank=-1, fastpath=False, delta_decay_factor=0.5) if residual == 2 else \
        dict(residual=1, ef=True, comp_rank=-1, fastpath=True)
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: T.WARMUP if s < warm else CT, **kw))
    g = torch.Generator(device=dev).manual_seed(1)
    k0 = [torch.randn(1, N, H, D, device=dev, dtype=torch.float16, generator=g) for _ in range(L)]
    v0 = [torch.randn(1, N, H, D, device=dev, dtype=torch.float16, generator=g) for _ in range(L)]
    ks = [[(k0[l] + 0.1 * torch.randn(1, N, H, D, device=dev, dtype=torch.float16, generator=g)) for l in range(L)] for _ in range(2)]
    vs = [[(v0[l] + 0.1 * torch.randn(1, N, H, D, device=dev, dtype=torch.float16, generator=g)) for l in range(L)] for _ in range(2)]
    q0 = torch.randn(1, N, H, D, device=dev, dtype=torch.float16, generator=g)
    out_ = torch.zeros(1, N, H, D, device=dev, dtype=torch.float16)
    lse_ = torch.zeros(1, N, H, 1, device=dev, dtype=torch.float32)
    ring.block_attention = lambda q, k, v, *a, **kw_: (out_, lse_)
    ring.update_out_and_lse = lambda out, lse, bo, bl, wait=None: (out_, lse_)
    ring._SteadyLayer._fast_ok = lambda self, q: False

    def step(i):
        cm.compact_set_step(i)
        for l in range(L):
            ring.compact_fwd(q0, ks[i & 1][l], vs[i & 1][l], causal=False, mod_idx=l, current_iter=i)
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        for i in range(warm + 3):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(warm + 3 + i)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
    assert lib.cfx_gate_errors(ctx) == 0
    ops = [e.xop for e in ring._xbuf.values() if e.xop is not None]
    print(json.dumps({"codec": codec, "residual": residual, "ms_per_step": round(ms, 4), "steps": args.steps,
                      "one_native_op_per_layer": len(ops) == L}), flush=True)
    xlayer.release()


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "runs": v}


def protocol():
    trees = [("parent", os.path.abspath(args.parent)), ("this", os.path.abspath(args.this))]
    runs = {(t, c, r): [] for t, _ in trees for c in ("BINARY", "INT2") for r in (2, 1)}
    for rep in range(args.repeats):
        for tname, tdir in trees:                      # parent first in every repeat
            for codec in ("BINARY", "INT2"):
                for residual in (2, 1):
                    cmd = [sys.executable, os.path.abspath(__file__), "--run", codec, str(residual), "--tree", tdir, "--steps", str(args.steps)]
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=tdir)
                    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                    if r.returncode != 0 or not line:
                        raise SystemExit(f"run failed ({tname} {codec} residual {residual}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
                    got = json.loads(line[-1])
                    runs[(tname, codec, residual)].append(got["ms_per_step"])
                    print(rep, tname, json.dumps(got), flush=True)
    res = {"what": "ms per denoise step through compact_fwd (ring gather schedule, lane off, no-op attention): FLUX shard (544, 3072), 57 "
                   "layers, 8 logical ranks looped back on one GPU; one process per run, parent tree first in every repeat, "
                   f"{args.repeats} repeats of {args.steps} steps after the warm-up; medians with min .. max",
           "parent_commit": args.parent_commit, "this_commit": args.this_commit, "rows": {}}
    for codec in ("BINARY", "INT2"):
        row = {f"{t}_residual{r}_ms": spread(runs[(t, codec, r)]) for t, _ in trees for r in (2, 1)}
        p2, t2, t1 = row["parent_residual2_ms"], row["this_residual2_ms"], row["this_residual1_ms"]
        row["residual2_this_over_parent"] = round(t2["median"] / p2["median"], 4)
        row["residual2_below_parent_by_more_than_the_spread"] = bool(t2["max"] < p2["min"])
        row["this_residual2_over_residual1"] = round(t2["median"] / t1["median"], 4)
        res["rows"][codec] = row
    print(json.dumps(res["rows"], indent=1))
    if args.json:
        json.dump(res, open(args.json, "w"), indent=1)


if args.run:
    one_run(args.run[0], int(args.run[1]))
elif args.parent:
    protocol()
else:
    ap.error("--run CODEC RESIDUAL, or --parent DIR")
