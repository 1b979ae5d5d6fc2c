"""What the native attention forward over all of a layer's K,V blocks (cfx_attn_fwd_blocks, configure(attention="native")) costs beside
the attention the default path runs - W fused SDPA calls and their merge -, measured on one MI355X in ONE session ->
profiles/attn_native_rows.json.

FLUX.1-dev shard as one rank of a ring of 8 sees it: q and blocks (1, 544, 24, 128), W = 8, fp16 and bf16, one process.  Rows:
  resource_rows  registers, scratch and LDS of every kernel of csrc/cfx_attn.hip, from the compiler's remarks (no GPU needed:
                 `python tools/attn_rows.py --resources` rewrites only these; tests/test_attn_fwd_f64.py compares them)
  layer          a layer's attention three ways on the same tensors, alternated REPS times (median and spread): W x SDPA + the merge
                 chain (cfx_attn_merge_ex, what the lean block loop issues), W x SDPA + the one-launch merge (attn_merge="once"), and
                 the ONE native launch; device events around ITERS passes -> us per layer, TFLOP/s (4 Sq W Sk H D flop), and the host
                 time to issue one layer into an empty queue
  qtile          the native launch with 64, 128 and 256 query rows a workgroup (cfx_set_attn_qtile), alternated like the forms above
  step           a 57-layer compact_fwd step, 8 logical ranks looped back, 1-bit codec: configure(lane="off") and the default lane;
                 attention sdpa + chain, sdpa + once and native alternated on the SAME bound layers; wall ms per step and host issue
                 us per layer
Nothing here asserts a time.  Run on the GPU:  python tools/attn_rows.py [--json profiles/attn_native_rows.json]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(REPO, "profiles", "attn_native_rows.json"))
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--layers", type=int, default=57)
ap.add_argument("--no-step", action="store_true", help="layer and qtile rows only")
ap.add_argument("--resources", action="store_true", help="rewrite resource_rows only (no GPU)")
args = ap.parse_args()


def resource_rows():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_usage as RU
    from compactfusion_amd import build as B
    rows = RU._one(B.ATTN_SRC[0])
    names = [re.sub(r"^void ", "", re.sub(r"\(.*$", "", d)) for d in RU.demangle([r["name"] for r in rows])]
    return {n: {k: r.get(k, 0) for k in ("vgpr", "agpr", "sgpr", "scratch", "lds", "occupancy")} for r, n in zip(rows, names) if n != "k_copy_probe"}


def load_json():
    try:
        with open(args.json) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def write_json(out):
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.json)


if args.resources:
    out = load_json()
    out["resource_rows"] = resource_rows()
    write_json(out)
    raise SystemExit(0)

os.environ["CFX_FAKE_RCCL_MODE"] = "loopback"
import torch
import compactfusion_amd
from compactfusion_amd import _lib, codecs as K, exchange
from compactfusion_amd.collector import collector
from compactfusion_amd.compact import attention as A, ring, main as cm, xlayer
from compactfusion_amd.compact.utils import CompactConfig, COMPACT_COMPRESS_TYPE as T
from compactfusion_amd.prof import Profiler

if not torch.cuda.is_available():
    raise SystemExit("tools/attn_rows.py measures on a GPU: none here (--resources needs none)")
B, S, H, D, W, L = 1, 544, 24, 128, 8, args.layers
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
lib = _lib.load()
ctx = K.context(0)
FLOP = 4.0 * S * W * S * H * D * B
MODES = (("sdpa_chain", "sdpa", "chain"), ("sdpa_once", "sdpa", "once"), ("native", "native", "chain"))


def sh():
    return torch.cuda.current_stream().cuda_stream


def stat(xs, nd=2):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def layer_rows(dtype, only_native=False):
    g = torch.Generator(device=dev).manual_seed(5)
    q = torch.randn(B, S, H, D, device=dev, dtype=dtype, generator=g)
    ks = [torch.randn(B, S, H, D, device=dev, dtype=dtype, generator=g) for _ in range(W)]
    vs = [torch.randn(B, S, H, D, device=dev, dtype=dtype, generator=g) for _ in range(W)]
    scale = D ** -0.5
    bf = _lib.ELEM_BF16 if dtype == torch.bfloat16 else 0
    sdpa = torch.ops.aten._scaled_dot_product_flash_attention
    qt, kts, vts = q.transpose(1, 2), [k.transpose(1, 2) for k in ks], [v.transpose(1, 2) for v in vs]
    acc = torch.empty(B, S, H, D, device=dev, dtype=torch.float32)
    out = torch.empty(B, S, H, D, device=dev, dtype=dtype)
    lse = torch.empty(B, S, H, device=dev, dtype=torch.float32)
    P = ctypes.c_void_p * W
    tabs = P(*[t.data_ptr() for t in ks]), P(*[t.data_ptr() for t in vs])
    res_out = {}

    def sdpa_chain():                                  # what `_blocks`' lean loop issues
        keep = []
        for i in range(W):
            r = sdpa(qt, kts[i], vts[i], 0.0, False, False, scale=scale)
            keep.append(r)
            fl = _lib.MERGE_BSHD | bf | (_lib.MERGE_FIRST if i == 0 else 0)
            rc = lib.cfx_attn_merge_ex(ctx, acc.data_ptr(), lse.data_ptr(), r[0].data_ptr(), r[1].data_ptr(), B, S, H, D, fl, None, 0,
                                       out.data_ptr() if i == W - 1 else None, sh())
            assert rc == 0, lib.cfx_last_error_string(ctx)
        res_out["sdpa_chain"] = out

    def sdpa_once():
        rs = [sdpa(qt, kts[i], vts[i], 0.0, False, False, scale=scale) for i in range(W)]
        res_out["sdpa_once"] = A.merge_blocks([r[0].transpose(1, 2) for r in rs], [r[1] for r in rs], dtype)[0]

    def native():
        res_out["native"] = A._attn_fwd_native(q, ks, vs, scale, tabs)[0]

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        dev_us = a.elapsed_time(b) / args.iters * 1e3
        host = 0.0
        for _ in range(20):                            # one layer at a time into an EMPTY queue
            t0 = time.perf_counter()
            fn()
            host += time.perf_counter() - t0
            torch.cuda.synchronize()
        return dev_us, host / 20 * 1e6

    forms = (("native", native),) if only_native else (("sdpa_chain", sdpa_chain), ("sdpa_once", sdpa_once), ("native", native))
    rows = {n: [] for n, _ in forms}
    for _ in range(args.reps):
        for n, fn in forms:
            rows[n].append(timed(fn))
    res = {}
    for n, _ in forms:
        us = [r[0] for r in rows[n]]
        res[n] = {"us_per_layer": stat(us), "TFLOPs": round(FLOP / (statistics.median(us) * 1e-6) / 1e12, 1),
                  "host_issue_us_per_layer": stat([r[1] for r in rows[n]], 1)}
    if not only_native:
        torch.cuda.synchronize()
        res["max_abs_difference_native_vs_sdpa_chain"] = float((res_out["native"].float() - res_out["sdpa_chain"].float()).abs().max())
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
        compactfusion_amd.configure(attention="sdpa", attn_merge="chain")
        with torch.cuda.stream(side):                                    # the caller on an ORDINARY stream
            step[0] = 0
            cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T.BINARY, residual=1, ef=True,
                                          comp_rank=-1, fastpath=True))
            fwd(); fwd(); fwd()
            torch.cuda.synchronize()
            exs = [e for e in ring._xbuf.values() if e.sig is not None]
            path = ("exchange lane" if exs and all(e.plan is not None and e.lane for e in exs) else
                    "layer op on the caller's stream" if exs and all(e.xop is not None for e in exs) else "other")
            rows = {m[0]: [] for m in MODES}
            launches = {}
            for _ in range(args.reps):
                for name, attention, merge in MODES:
                    compactfusion_amd.configure(attention=attention, attn_merge=merge)
                    fwd(); torch.cuda.synchronize()
                    n0 = A.attn_fwd_launches(0)
                    rows[name].append(timed())
                    launches[name] = (A.attn_fwd_launches(0) - n0) / (2 * args.steps + 1) / L
            compactfusion_amd.configure(attention="sdpa", attn_merge="chain")
        res[leg] = {"path": path, "steady_layers": len(ring._steady), "native_launches_per_layer": launches}
        for name, _, _ in MODES:
            wall, host = [r[0] for r in rows[name]], [r[1] for r in rows[name]]
            res[leg][name] = {"wall_ms_per_step": stat(wall, 3), "host_issue_us_per_layer": stat([h * 1e3 / L for h in host], 1)}
        assert lib.cfx_gate_errors(ctx) == 0
        cm._drop_kv_exchanges()
        for e in ring._xbuf.values():
            e.close()
        ring._xbuf.clear(); ring._steady.clear(); ring._lane_ok.clear()
        xlayer.set_p2p_loopback(False)
        exchange.set_comm_factory(None)
    return res


prev = load_json()
out = {
    "what": "cfx_attn_fwd_blocks (one native launch over all K,V blocks) beside W fused SDPA calls and their merge, one MI355X, one session",
    "device": torch.cuda.get_device_name(0),
    "shape": {"q_and_blocks": [B, S, H, D], "W": W, "layers": L},
    "flop_per_layer": FLOP,
    "iters": args.iters, "reps": args.reps, "steps": args.steps,
    "resource_rows": prev.get("resource_rows") or resource_rows(),
    "layer": {}, "qtile": {}, "step": {},
}
for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
    out["layer"][name] = layer_rows(dtype)
    print(name, json.dumps(out["layer"][name]), flush=True)
rows = {qt: {"fp16": [], "bf16": []} for qt in (64, 128, 256)}
try:
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        for _ in range(2):
            for qt in rows:
                assert lib.cfx_set_attn_qtile(ctx, qt) == 0
                rows[qt][name].append(layer_rows(dtype, only_native=True)["native"])
finally:
    lib.cfx_set_attn_qtile(ctx, 0)
for qt in rows:
    out["qtile"][str(qt)] = {name: {"us_per_layer_medians": [r["us_per_layer"]["median"] for r in rs], "TFLOPs": max(r["TFLOPs"] for r in rs)}
                             for name, rs in rows[qt].items()}
    print("qtile", qt, json.dumps(out["qtile"][str(qt)]), flush=True)
if not args.no_step:
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        out["step"][name] = step_rows(dtype)
        print(name, json.dumps(out["step"][name]), flush=True)
write_json(out)
