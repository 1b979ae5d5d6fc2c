"""What merging a layer's attention blocks in ONE launch (cfx_attn_merge_many, configure(attn_merge="once")) costs beside the chain of
one launch per block (cfx_attn_merge_ex, the default), measured on one MI355X in ONE session -> profiles/attn_merge_many_rows.json.

FLUX.1-dev shard as one rank of a ring of 8 sees it: blocks (1, 544, 24, 128), W = 8, fp16 and bf16.  Rows:
  kernels   the 8-launch chain (7 launches into the fp32 accumulator, the last writing the 16-bit result: what the lean block loop issues)
            against the one launch, on the same block tensors, `warm` (one set of blocks, resident in the caches after the first pass, as
            the SDPA kernel leaves them for the merge that follows it) and `cold` (sets rotated so that every pass reads from HBM: more
            bytes than the 256 MiB last-level cache holds); device events around ITERS passes, the two forms alternated REPS times
            (median and spread), and - in a pass of their own - the kernels' own times from the library's launch records
  copy      cfx_copy_probe moving as many bytes as the one launch moves (its reads + its writes), warm and cold
  step      a 57-layer compact_fwd step with PyTorch-ROCm's fused SDPA, 8 logical ranks looped back (tests/fake_rccl in loopback mode /
            the looped-back peer-to-peer arena), 1-bit codec: configure(lane="off") and the default lane, attn_merge chain and once
            alternated on the SAME bound layers; wall ms per step and host issue us per layer (one step at a time into an empty queue)
Nothing here asserts a time.  Run on the GPU:  python tools/merge_rows.py [--json profiles/attn_merge_many_rows.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(REPO, "profiles", "attn_merge_many_rows.json"))
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--layers", type=int, default=57)
ap.add_argument("--no-step", action="store_true", help="kernel and copy rows only")
args = ap.parse_args()

os.environ["CFX_FAKE_RCCL_MODE"] = "loopback"
import compactfusion_amd
from compactfusion_amd import _lib, codecs as K, exchange
from compactfusion_amd.collector import collector
from compactfusion_amd.compact import ring, main as cm, xlayer
from compactfusion_amd.compact.utils import CompactConfig, COMPACT_COMPRESS_TYPE as T
from compactfusion_amd.prof import Profiler

if not torch.cuda.is_available():
    raise SystemExit("tools/merge_rows.py measures on a GPU: none here")
B, S, H, D, W, L = 1, 544, 24, 128, 8, args.layers
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
lib = _lib.load()
ctx = K.context(0)
KID_ATTN_MERGE = 30
ROWS = B * S * H
MOVED = W * (ROWS * D * 2 + ROWS * 4) + ROWS * D * 2 + ROWS * 4          # bytes the one launch reads + writes
CHAIN_MOVED = MOVED + 2 * (W - 1) * ROWS * D * 4 + 2 * (W - 1) * ROWS * 4      # ... and the chain: the fp32 accumulator written 7 x and read 7 x, lse too
COLD_SETS = 12                                                            # 12 x 26.8 MB of blocks: more than the 256 MiB last-level cache


def sh():
    return torch.cuda.current_stream().cuda_stream


def make_sets(dtype, n_sets):
    g = torch.Generator(device=dev).manual_seed(5)
    sets = []
    for _ in range(n_sets):
        outs = [torch.randn(B, S, H, D, device=dev, dtype=dtype, generator=g) for _ in range(W)]
        lses = [torch.randn(B, H, S, device=dev, dtype=torch.float32, generator=g) for _ in range(W)]
        P = ctypes.c_void_p * W
        sets.append((outs, lses, P(*[t.data_ptr() for t in outs]), P(*[t.data_ptr() for t in lses])))
    return sets


def kernel_rows(dtype):
    bf = _lib.ELEM_BF16 if dtype == torch.bfloat16 else 0
    acc = torch.empty(B, S, H, D, device=dev, dtype=torch.float32)
    out = torch.empty(B, S, H, D, device=dev, dtype=dtype)
    out2 = torch.empty(B, S, H, D, device=dev, dtype=dtype)
    lse = torch.empty(B, S, H, device=dev, dtype=torch.float32)
    lse2 = torch.empty(B, S, H, device=dev, dtype=torch.float32)
    sets = make_sets(dtype, COLD_SETS)

    def chain(st):
        outs, lses = st[0], st[1]
        for i in range(W):
            fl = _lib.MERGE_BSHD | bf | (_lib.MERGE_FIRST if i == 0 else 0)
            rc = lib.cfx_attn_merge_ex(ctx, acc.data_ptr(), lse.data_ptr(), outs[i].data_ptr(), lses[i].data_ptr(), B, S, H, D, fl, None, 0,
                                       out.data_ptr() if i == W - 1 else None, sh())
            assert rc == 0, lib.cfx_last_error_string(ctx)

    def once(st):
        rc = lib.cfx_attn_merge_many(ctx, W, st[2], st[3], B, S, H, D, _lib.MERGE_BSHD | bf, out2.data_ptr(), lse2.data_ptr(), sh())
        assert rc == 0, lib.cfx_last_error_string(ctx)

    def timed(fn, use):
        for i in range(len(use) + 3):
            fn(use[i % len(use)])
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(args.iters):
            fn(use[i % len(use)])
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters * 1e3                      # us per pass (launch gaps included: what a stream pays)

    def kernel_time(fn, use):
        """the kernels' own execution time per pass, from the library's launch records (events on the dispatch packets)"""
        n = 16
        assert lib.cfx_profile_enable(ctx, 8 * W * n, 1 << KID_ATTN_MERGE, 1) == 0
        for i in range(n):
            fn(use[i % len(use)])
        torch.cuda.synchronize()
        ids, ms = (ctypes.c_int * (8 * W * n))(), (ctypes.c_float * (8 * W * n))()
        k = lib.cfx_profile_read(ctx, ids, ms, 8 * W * n)
        lib.cfx_profile_enable(ctx, 0, 0, 1)
        return sum(ms[i] for i in range(k)) / n * 1e3, k // n

    res = {}
    for res_name, use in (("warm", sets[:1]), ("cold", sets)):
        c, o = [], []
        for _ in range(args.reps):
            c.append(timed(chain, use))
            o.append(timed(once, use))
        ck, cn = kernel_time(chain, use)
        ok, on = kernel_time(once, use)
        res[res_name] = {
            "chain_us_per_layer": {"median": round(statistics.median(c), 2), "min": round(min(c), 2), "max": round(max(c), 2), "launches": cn},
            "once_us_per_layer": {"median": round(statistics.median(o), 2), "min": round(min(o), 2), "max": round(max(o), 2), "launches": on},
            "chain_kernel_us_per_layer": round(ck, 2), "once_kernel_us_per_layer": round(ok, 2),
            "once_kernel_GBps": round(MOVED / (ok * 1e-6) / 1e9, 1), "chain_kernel_GBps": round(CHAIN_MOVED / (ck * 1e-6) / 1e9, 1),
        }
    # the two forms on the same inputs (last cold set): how far apart the 16-bit results are
    chain(sets[-1]); once(sets[-1]); torch.cuda.synchronize()
    res["max_abs_difference_of_the_16_bit_results"] = float((out.float() - out2.float()).abs().max())
    res["results_equal_bitwise_fraction"] = float((out.view(torch.int16) == out2.view(torch.int16)).float().mean())
    # copy probe of the one launch's bytes
    half = (MOVED // 2 + 15) // 16 * 16
    srcs = [torch.empty(half, device=dev, dtype=torch.uint8).random_(0, 255) for _ in range(2 * COLD_SETS)]
    dst = torch.empty(half, device=dev, dtype=torch.uint8)

    def copy(src):
        assert lib.cfx_copy_probe(ctx, dst.data_ptr(), src.data_ptr(), half, sh()) == 0
    for res_name, use in (("warm", srcs[:1]), ("cold", srcs)):
        t = [timed(copy, use) for _ in range(args.reps)]
        res[res_name]["copy_probe_us_same_bytes"] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
        res[res_name]["copy_probe_GBps"] = round(2 * half / (statistics.median(t) * 1e-6) / 1e9, 1)
    return res


# ---- the 57-layer step -----------------------------------------------------------------------------------------------------------------
def step_rows(dtype):
    ring.dist.get_rank = lambda g=None: 0
    ring.dist.get_world_size = lambda g=None: W
    ring.dist.all_gather_into_tensor = lambda recv, send, group=None: recv.view(W, -1).copy_(send.view(1, -1).expand(W, -1))
    sys.path.insert(0, os.path.join(REPO, "tests", "fake_rccl"))
    import build as fake_build
    fake = fake_build.build()

    class LoopComm:
        def __init__(self, group, device):
            c = K.context(device)
            assert lib.cfx_rccl_load(fake.encode()) == 0
            uid = ctypes.create_string_buffer(128)
            assert lib.cfx_comm_unique_id(c, uid) == 0
            self.handle = lib.cfx_comm_create(c, uid, W, 0)
            assert self.handle
    Profiler.instance().disable()
    collector.init(collector.Collector("/tmp/none", enabled=False))
    g = torch.Generator(device=dev).manual_seed(1)
    qs = [torch.randn(B, S, H, D, device=dev, dtype=dtype, generator=g) for _ in range(L)]
    k0 = [torch.randn(B, S, H, D, device=dev, dtype=dtype, generator=g) for _ in range(L)]
    v0 = [torch.randn(B, S, H, D, device=dev, dtype=dtype, generator=g) for _ in range(L)]
    drift = [[0.1 * torch.randn(B, S, H, D, device=dev, dtype=dtype, generator=g) for _ in range(L)] for _ in range(2)]
    ks = [[(k0[l] + drift[s][l]) for l in range(L)] for s in range(2)]
    vs = [[(v0[l] - drift[s][l]) for l in range(L)] for s in range(2)]
    torch.cuda.synchronize()
    step = [0]

    def fwd():
        i = step[0]
        step[0] += 1
        cm.compact_set_step(i)
        for l in range(L):
            ring.compact_fwd(qs[l], ks[i & 1][l], vs[i & 1][l], causal=False, mod_idx=l, current_iter=i)

    def timed():
        fwd(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fwd()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.steps * 1e3
        host = 0.0
        for _ in range(args.steps):                                      # one step at a time into an EMPTY queue
            th = time.perf_counter()
            fwd()
            host += time.perf_counter() - th
            torch.cuda.synchronize()
        return wall, host / args.steps * 1e3

    res = {}
    side = torch.cuda.Stream(dev)
    for leg, lane_mode in (("lane_off", "off"), ("default_lane", "auto")):
        os.environ["CFX_RING_SCHEDULE"] = "gather"
        os.environ["CFX_LANE"] = lane_mode
        os.environ.pop("CFX_RING_EXCHANGE_STREAM", None)
        if lane_mode == "off":
            os.environ.pop("CFX_RING_EXCHANGE", None)
            exchange.set_comm_factory(None)
            xlayer.set_p2p_loopback(True)
        else:
            os.environ["CFX_RING_EXCHANGE"] = "native"
            exchange.set_comm_factory(LoopComm)
        ring._xbuf.clear(); ring._steady.clear(); ring._lane_ok.clear()
        compactfusion_amd.configure(attn_merge="chain")
        with torch.cuda.stream(side):                                    # the caller on an ORDINARY stream
            step[0] = 0
            cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T.BINARY, residual=1, ef=True,
                                          comp_rank=-1, fastpath=True))
            fwd(); fwd(); fwd()
            torch.cuda.synchronize()
            exs = [e for e in ring._xbuf.values() if e.sig is not None]
            path = ("exchange lane" if exs and all(e.plan is not None and e.lane for e in exs) else
                    "layer op on the caller's stream" if exs and all(e.xop is not None for e in exs) else "other")
            rows = {"chain": [], "once": []}
            for _ in range(args.reps):
                for mode in ("chain", "once"):
                    compactfusion_amd.configure(attn_merge=mode)
                    fwd(); torch.cuda.synchronize()
                    rows[mode].append(timed())
            compactfusion_amd.configure(attn_merge="chain")
        res[leg] = {"path": path, "steady_layers": len(ring._steady), "lean_loop": all(st._fast is True for st in ring._steady.values())}
        for mode in ("chain", "once"):
            wall, host = [r[0] for r in rows[mode]], [r[1] for r in rows[mode]]
            res[leg][mode] = {"wall_ms_per_step": {"median": round(statistics.median(wall), 3), "min": round(min(wall), 3), "max": round(max(wall), 3)},
                              "host_issue_us_per_layer": {"median": round(statistics.median(host) * 1e3 / L, 1), "min": round(min(host) * 1e3 / L, 1),
                                                          "max": round(max(host) * 1e3 / L, 1)}}
        assert lib.cfx_gate_errors(ctx) == 0
        cm._drop_kv_exchanges()
        for e in ring._xbuf.values():
            e.close()
        ring._xbuf.clear(); ring._steady.clear(); ring._lane_ok.clear()
        xlayer.set_p2p_loopback(False)
        exchange.set_comm_factory(None)
    return res


out = {
    "what": "cfx_attn_merge_many (one launch) beside the cfx_attn_merge_ex chain (one launch per block), one MI355X, one session",
    "device": torch.cuda.get_device_name(0),
    "shape": {"blocks": [B, S, H, D], "W": W, "layers": L},
    "bytes_per_layer": {"one_launch_reads_plus_writes": MOVED, "chain_reads_plus_writes": CHAIN_MOVED},
    "iters": args.iters, "reps": args.reps, "steps": args.steps,
    "kernels": {}, "step": {},
}
for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
    out["kernels"][name] = kernel_rows(dtype)
    print(name, json.dumps(out["kernels"][name]), flush=True)
if not args.no_step:
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        out["step"][name] = step_rows(dtype)
        print(name, json.dumps(out["step"][name]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
with open(args.json, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.json)
