"""What a compact_fwd layer WITH joint tensors costs on the steady layer (configure(joint="steady")) beside the general path every joint call
took before, and what the one launch over K,V blocks of unequal length (cfx_attn_fwd_blocks_var) costs beside the equal-length launch -
measured on one MI355X in ONE session, one process -> profiles/attn_joint_rows.json.

Shapes: FLUX as xDiT runs it - K,V shards (1, 512, 24, 128), W = 8, joint (text) K,V of 512 keys with joint_strategy="front", queries
[text ; image shard] (1, 1024, 24, 128) -, fp16 and bf16.
  resource_rows  registers, scratch and LDS of every kernel of csrc/cfx_attn_var.hip, from the compiler's remarks (no GPU needed:
                 `python tools/attn_joint_rows.py --resources` rewrites only these)
  layer          a layer's attention alone on resident tensors, the forms alternated --reps times, median (min - max): the general
                 path (block_attention + update_out_and_lse per block from Python, block 0 = cat([joint, own]) - what `attend` runs), the
                 steady sdpa loop with the merge chain and with the one-launch merge, and the ONE var launch over [joint, own, peers...]
  walk           the var launch against cfx_attn_fwd_blocks on the same 9 x 512 keys in equal blocks: what per-block lengths cost the walk
  step           the 57-layer step through compact_fwd with joint tensors (1-bit codec, W logical ranks looped back), configure(lane="off")
                 and the default lane, joint="general" and joint="steady" with sdpa + chain, sdpa + once and native; host issue time per layer
Nothing here asserts a time.  Run on the GPU:  python tools/attn_joint_rows.py [--json profiles/attn_joint_rows.json]"""
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
ap.add_argument("--json", default=os.path.join(REPO, "profiles", "attn_joint_rows.json"))
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--layers", type=int, default=57)
ap.add_argument("--no-step", action="store_true", help="layer and walk rows only")
ap.add_argument("--resources", action="store_true", help="rewrite resource_rows only (no GPU)")
args = ap.parse_args()


def resource_rows():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_usage as RU
    from compactfusion_amd import build as B
    rows = RU._one(B.ATTN_VAR_SRC[0])
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
    raise SystemExit("tools/attn_joint_rows.py measures on a GPU: none here (--resources needs none)")
B, S, SJ, H, D, W, L = 1, 512, 512, 24, 128, 8, args.layers
SQ = SJ + S
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
lib = _lib.load()
ctx = K.context(0)
FLOP = 4.0 * SQ * (SJ + W * S) * H * D * B
FORMS = (("general", "general", "sdpa", "chain"), ("steady_sdpa_chain", "steady", "sdpa", "chain"), ("steady_sdpa_once", "steady", "sdpa", "once"),
         ("steady_native", "steady", "native", "chain"))


def sh():
    return torch.cuda.current_stream().cuda_stream


def stat(xs, nd=2):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def timed(fn):
    for _ in range(3):
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
    for _ in range(10):                                # one layer at a time into an EMPTY queue
        t0 = time.perf_counter()
        fn()
        host += time.perf_counter() - t0
        torch.cuda.synchronize()
    return dev_us, host / 10 * 1e6


def alternate(forms):
    rows = {n: [] for n, _ in forms}
    for _ in range(args.reps):
        for n, fn in forms:
            rows[n].append(timed(fn))
    res = {}
    for n, _ in forms:
        us = [r[0] for r in rows[n]]
        res[n] = {"us_per_layer": stat(us), "TFLOPs": round(FLOP / (statistics.median(us) * 1e-6) / 1e12, 1),
                  "host_issue_us_per_layer": stat([r[1] for r in rows[n]], 1)}
    return res


def layer_rows(dtype):
    g = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda n: torch.randn(B, n, H, D, device=dev, dtype=dtype, generator=g)      # noqa: E731
    q, jk, jv = rnd(SQ), rnd(SJ), rnd(SJ)
    ks, vs = [rnd(S) for _ in range(W)], [rnd(S) for _ in range(W)]
    scale = D ** -0.5
    bf = _lib.ELEM_BF16 if dtype == torch.bfloat16 else 0
    sdpa = torch.ops.aten._scaled_dot_product_flash_attention
    qt = q.transpose(1, 2)
    acc = torch.empty(B, SQ, H, D, device=dev, dtype=torch.float32)
    out = torch.empty(B, SQ, H, D, device=dev, dtype=dtype)
    lse = torch.empty(B, SQ, H, device=dev, dtype=torch.float32)
    n = W + 1
    P = ctypes.c_void_p * n
    bk, bv = [jk] + ks, [jv] + vs
    tabs = P(*[t.data_ptr() for t in bk]), P(*[t.data_ptr() for t in bv]), (ctypes.c_int * n)(*[t.shape[1] for t in bk])
    res_out = {}

    def blocks_t():                                    # block 0 = [joint ; own], concatenated by every call as compact_fwd does
        k0, v0 = torch.cat([jk, ks[0]], dim=1), torch.cat([jv, vs[0]], dim=1)
        return [k0] + ks[1:], [v0] + vs[1:]

    def general():                                     # what `attend` of the general path issues per block
        o = l = None
        kk, vv = blocks_t()
        for i in range(W):
            bo, bl = A.block_attention(q, kk[i], vv[i], 0.0, scale, causal=False)
            o, l = A.update_out_and_lse(o, l, bo, bl)
        res_out["general"] = o.to(dtype)

    def sdpa_chain():                                  # what `_blocks`' lean loop issues
        keep = []
        kk, vv = blocks_t()
        for i in range(W):
            r = sdpa(qt, kk[i].transpose(1, 2), vv[i].transpose(1, 2), 0.0, False, False, scale=scale)
            keep.append(r)
            fl = _lib.MERGE_BSHD | bf | (_lib.MERGE_FIRST if i == 0 else 0)
            rc = lib.cfx_attn_merge_ex(ctx, acc.data_ptr(), lse.data_ptr(), r[0].data_ptr(), r[1].data_ptr(), B, SQ, H, D, fl, None, 0,
                                       out.data_ptr() if i == W - 1 else None, sh())
            assert rc == 0, lib.cfx_last_error_string(ctx)
        res_out["steady_sdpa_chain"] = out

    def sdpa_once():
        kk, vv = blocks_t()
        rs = [sdpa(qt, kk[i].transpose(1, 2), vv[i].transpose(1, 2), 0.0, False, False, scale=scale) for i in range(W)]
        res_out["steady_sdpa_once"] = A.merge_blocks([r[0].transpose(1, 2) for r in rs], [r[1] for r in rs], dtype)[0]

    def native():
        res_out["steady_native"] = A._attn_fwd_native_var(q, bk, bv, scale, tabs)[0]

    res = alternate((("general", general), ("steady_sdpa_chain", sdpa_chain), ("steady_sdpa_once", sdpa_once), ("steady_native", native)))
    torch.cuda.synchronize()
    res["max_abs_difference_native_vs_general"] = float((res_out["steady_native"].float() - res_out["general"].float()).abs().max())
    # the walk: the same 9 x 512 keys through both entry points (all lengths equal: the var launch pays only its per-block bookkeeping)
    t2 = tabs[0], tabs[1]
    eq = lambda: A._attn_fwd_native(q, bk, bv, scale, t2)          # noqa: E731
    walk = alternate((("equal_length_launch", eq), ("var_launch", native)))
    a, b = eq(), A._attn_fwd_native_var(q, bk, bv, scale, tabs)
    torch.cuda.synchronize()
    walk["same_bits"] = bool(torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].contiguous().view(torch.int32), b[1].contiguous().view(torch.int32)))
    return res, walk


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
    rnd = lambda n: torch.randn(B, n, H, D, device=dev, dtype=dtype, generator=g)      # noqa: E731
    qs, jks, jvs = [rnd(SQ) for _ in range(L)], [rnd(SJ) for _ in range(L)], [rnd(SJ) for _ in range(L)]
    k0, v0 = [rnd(S) for _ in range(L)], [rnd(S) for _ in range(L)]
    drift = [[0.1 * rnd(S) for _ in range(L)] for _ in range(2)]
    ks = [[(k0[l] + drift[s][l]) for l in range(L)] for s in range(2)]
    vs = [[(v0[l] - drift[s][l]) for l in range(L)] for s in range(2)]
    torch.cuda.synchronize()
    step = [0]

    def fwd():
        i = step[0]
        step[0] += 1
        cm.compact_set_step(i)
        for l in range(L):
            ring.compact_fwd(qs[l], ks[i & 1][l], vs[i & 1][l], causal=False, mod_idx=l, current_iter=i,
                             joint_tensor_key=jks[l], joint_tensor_value=jvs[l], joint_strategy="front")

    def timed_steps():
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
        compactfusion_amd.configure(joint="general", attention="sdpa", attn_merge="chain")
        with torch.cuda.stream(side):                                    # the caller on an ORDINARY stream
            step[0] = 0
            cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T.BINARY, residual=1, ef=True,
                                          comp_rank=-1, fastpath=True))
            fwd(); fwd(); fwd()
            torch.cuda.synchronize()
            exs = [e for e in ring._xbuf.values() if e.sig is not None]
            path = ("exchange lane" if exs and all(e.plan is not None and e.lane for e in exs) else
                    "layer op on the caller's stream" if exs and all(e.xop is not None for e in exs) else "other")
            rows = {f[0]: [] for f in FORMS}
            launches = {}
            for _ in range(args.reps):
                for name, joint, attention, merge in FORMS:
                    compactfusion_amd.configure(joint=joint, attention=attention, attn_merge=merge)
                    fwd(); torch.cuda.synchronize()
                    n0 = A.attn_fwd_launches(0)
                    rows[name].append(timed_steps())
                    launches[name] = (A.attn_fwd_launches(0) - n0) / (2 * args.steps + 1) / L
            compactfusion_amd.configure(joint="general", attention="sdpa", attn_merge="chain")
        res[leg] = {"path": path, "steady_layers": len(ring._steady), "native_launches_per_layer": launches}
        for name, _, _, _ in FORMS:
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
    "what": "compact_fwd with joint tensors on the steady layer (configure(joint='steady')) beside the general path, and cfx_attn_fwd_blocks_var "
            "beside cfx_attn_fwd_blocks, one MI355X, one session",
    "device": torch.cuda.get_device_name(0),
    "shape": {"q": [B, SQ, H, D], "kv_shard": [B, S, H, D], "joint": [B, SJ, H, D], "joint_strategy": "front", "W": W, "layers": L},
    "flop_per_layer": FLOP,
    "iters": args.iters, "reps": args.reps, "steps": args.steps,
    "resource_rows": prev.get("resource_rows") or resource_rows(),
    "layer": {}, "walk": {}, "step": {},
    "not_measured": ["live peers (the W ranks are looped back on one GPU)", "W other than 8", "joint_strategy='rear' at SD3's shapes", "other head dims and shard lengths",
                     "the step under a hipGraph", "a kernel trace or hardware counters"],
}
for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
    out["layer"][name], out["walk"][name] = layer_rows(dtype)
    print(name, json.dumps(out["layer"][name]), json.dumps(out["walk"][name]), flush=True)
if not args.no_step:
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        out["step"][name] = step_rows(dtype)
        print(name, json.dumps(out["step"][name]), flush=True)
write_json(out)
