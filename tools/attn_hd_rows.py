"""What the one-launch attention costs at the head dims between 64 and 128 (cfx_attn_fwd_blocks_hd) beside what a caller could do before
it - measured on one MI355X in ONE session, one process -> profiles/attn_hd_rows.json.

Shapes: PixArt 512^2 as BASELINE config 2 runs it - K,V shards (2, 512, 16, 72), W = 2 -, PixArt 1024^2 at W = 8 - shards (2, 512, 16, 72) -,
and one D = 88 row (HunyuanDiT's heads: shards (2, 512, 16, 88), W = 8); the queries are a rank's own shard.  fp16.
  resource_rows  registers, scratch and LDS of every kernel of csrc/cfx_attn_hd.hip, from the compiler's remarks (no GPU needed:
                 `python tools/attn_hd_rows.py --resources` rewrites only these)
  layer          a layer's attention alone on resident tensors, the forms alternated --reps times, median (min - max), device events
                 around --iters layers back to back:
                   cat_sdpa         (a) the patch path as it was: two torch.cat(...).contiguous() copies of the W states, one fused SDPA call
                   padded_var       (b) cfx_attn_fwd_blocks_var on q and the states zero-padded to D = 128 - what a caller could do before -,
                                    the padding done once outside the timed region
                   padded_var_copy  (b) with the 2 W + 1 padding copies inside it
                   hd               (c) ONE cfx_attn_fwd_blocks_hd launch on the states where they lie
  step           the patch-parallel step through patch_gather_fwd (synchronous raw gather, the W ranks looped back on one GPU), --layers
                 layers, configure(attention="sdpa") and "native"
Nothing here asserts a time.  Run on the GPU:  python tools/attn_hd_rows.py [--json profiles/attn_hd_rows.json]"""
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
ap.add_argument("--json", default=os.path.join(REPO, "profiles", "attn_hd_rows.json"))
ap.add_argument("--iters", type=int, default=56)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--layers", type=int, default=28)
ap.add_argument("--no-step", action="store_true", help="layer rows only")
ap.add_argument("--resources", action="store_true", help="rewrite resource_rows only (no GPU)")
args = ap.parse_args()


def resource_rows():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_usage as RU
    from compactfusion_amd import build as B
    rows = RU._one(B.ATTN_HD_SRC[0])
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

import torch
import compactfusion_amd
from compactfusion_amd import _lib, codecs as K
from compactfusion_amd.collector import collector
from compactfusion_amd.compact import attention as A, main as cm
from compactfusion_amd.compact.patchpara import fwd as PF
from compactfusion_amd.compact.utils import CompactConfig, COMPACT_COMPRESS_TYPE as T
from compactfusion_amd.compact.patchpara.df_utils import PatchConfig
from compactfusion_amd.prof import Profiler

if not torch.cuda.is_available():
    raise SystemExit("tools/attn_hd_rows.py measures on a GPU: none here (--resources needs none)")
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
lib = _lib.load()
ctx = K.context(0)
dtype = torch.float16
SHAPES = (("pixart512_w2_d72", 2, 512, 16, 72, 2), ("pixart1024_w8_d72", 2, 512, 16, 72, 8), ("hunyuan_w8_d88", 2, 512, 16, 88, 8))


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
    return a.elapsed_time(b) / args.iters * 1e3


def alternate(forms, flop):
    rows = {n: [] for n, _ in forms}
    for _ in range(args.reps):
        for n, fn in forms:
            rows[n].append(timed(fn))
    return {n: {"us_per_layer": stat(rows[n]), "TFLOPs": round(flop / (statistics.median(rows[n]) * 1e-6) / 1e12, 1)} for n, _ in forms}


def layer_rows(B, S, H, D, W):
    g = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda: torch.randn(B, S, H, D, device=dev, dtype=dtype, generator=g)      # noqa: E731
    q = rnd()
    ks, vs = [rnd() for _ in range(W)], [rnd() for _ in range(W)]
    scale = D ** -0.5
    pad = lambda t: torch.nn.functional.pad(t, (0, 128 - D)).contiguous()             # noqa: E731
    pq, pks, pvs = pad(q), [pad(t) for t in ks], [pad(t) for t in vs]
    P = ctypes.c_void_p * W
    sks = (ctypes.c_int * W)(*([S] * W))
    tabs = P(*[t.data_ptr() for t in ks]), P(*[t.data_ptr() for t in vs]), sks
    ptabs = P(*[t.data_ptr() for t in pks]), P(*[t.data_ptr() for t in pvs]), sks
    res_out = {}

    def cat_sdpa():
        gk, gv = torch.cat(ks, dim=1).contiguous(), torch.cat(vs, dim=1).contiguous()
        res_out["cat_sdpa"] = A.block_attention(q, gk, gv, 0.0, scale, causal=False)[0]

    def padded_var():
        res_out["padded_var"] = A._attn_fwd_native_var(pq, pks, pvs, scale, ptabs)[0]

    def padded_var_copy():
        q2, k2, v2 = pad(q), [pad(t) for t in ks], [pad(t) for t in vs]
        A._attn_fwd_native_var(q2, k2, v2, scale)

    def hd():
        res_out["hd"] = A._attn_fwd_native_var(q, ks, vs, scale, tabs)[0]

    res = alternate((("cat_sdpa", cat_sdpa), ("padded_var", padded_var), ("padded_var_copy", padded_var_copy), ("hd", hd)), 4.0 * S * W * S * H * D * B)
    torch.cuda.synchronize()
    res["hd_equals_padded_var_bits"] = bool(torch.equal(res_out["hd"].view(torch.int16), res_out["padded_var"][..., :D].contiguous().view(torch.int16)))
    res["max_abs_difference_hd_vs_cat_sdpa"] = float((res_out["hd"].float() - res_out["cat_sdpa"].float()).abs().max())
    return res


def step_rows(B, S, H, D, W):
    """the step through patch_gather_fwd: synchronous raw gather, every rank's shard this rank's own (looped back)"""
    L = args.layers
    PF.dist.get_rank = lambda g=None: 0
    PF.dist.get_world_size = lambda g=None: W

    def loop_back(recv, send, group=None, async_op=False):
        recv.view(W, -1).copy_(send.view(1, -1).expand(W, -1))
    PF.dist.all_gather_into_tensor = loop_back
    Profiler.instance().disable()
    collector.init(collector.Collector("/tmp/none", enabled=False))
    cm.compact_init(CompactConfig(enabled=True, override_with_patch_gather_fwd=True, patch_gather_fwd_config=PatchConfig(False, False, 1),
                                  compress_func=lambda l, s: T.WARMUP, residual=1, ef=True, comp_rank=-1, fastpath=True))
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda: torch.randn(B, S, H, D, device=dev, dtype=dtype, generator=g)      # noqa: E731
    qs, ks, vs = [rnd() for _ in range(L)], [rnd() for _ in range(L)], [rnd() for _ in range(L)]
    step = [0]

    def fwd():
        i = step[0]
        step[0] += 1
        cm.compact_set_step(i)
        for l in range(L):
            PF.patch_gather_fwd(qs[l], ks[l], vs[l], causal=False, mod_idx=l, current_iter=i)

    def timed_steps():
        fwd(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fwd()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3
    rows, launches = {"sdpa": [], "native": []}, {}
    for _ in range(args.reps):
        for attention in ("sdpa", "native"):
            compactfusion_amd.configure(attention=attention)
            n0 = A.attn_fwd_launches(0)
            rows[attention].append(timed_steps())
            launches[attention] = (A.attn_fwd_launches(0) - n0) / (args.steps + 1) / L
    compactfusion_amd.configure(attention="sdpa")
    return {"layers": L, "native_launches_per_layer": launches, **{a: {"wall_ms_per_step": stat(rows[a], 3)} for a in rows}}


prev = load_json()
out = {
    "what": "cfx_attn_fwd_blocks_hd (head dims 72 .. 120) beside cat + SDPA and beside cfx_attn_fwd_blocks_var on tensors zero-padded to D = 128; "
            "patch_gather_fwd with attention sdpa / native; one MI355X, one session, one process",
    "device": torch.cuda.get_device_name(0),
    "dtype": "fp16", "iters": args.iters, "reps": args.reps, "steps": args.steps,
    "resource_rows": prev.get("resource_rows") or resource_rows(),
    "layer": {}, "step": {},
    "not_measured": ["live peers (the W ranks are looped back on one GPU)", "the compressed (compact / displaced) and the async gather modes in the step rows",
                     "joint tensors", "bf16", "head dims other than 72 and 88", "query tiles other than 128", "a kernel trace or hardware counters"],
}
for name, B, S, H, D, W in SHAPES:
    out["layer"][name] = dict(shape={"q": [B, S, H, D], "kv_shard": [B, S, H, D], "W": W}, **layer_rows(B, S, H, D, W))
    print(name, json.dumps(out["layer"][name]), flush=True)
    write_json(out)
if not args.no_step:
    for name, B, S, H, D, W in SHAPES[:2]:
        out["step"][name] = step_rows(B, S, H, D, W)
        print(name, json.dumps(out["step"][name]), flush=True)
write_json(out)
