"""Two commits' `tools/overlap_bench.py` runs side by side (profiles/bf16_overlap.json).

Input: a directory of `overlap_bench.py --json` files named  <tree>_<dtype>_<repeat>.json  with tree in {parent, new} and dtype in
{fp16, bf16} - one process per file, the processes of the two checkouts alternating in one GPU call (which tree goes first alternates
from repeat to repeat when the caller runs them so; say it with --order).  Output: per dtype, tree and leg the wall and host-issue ms per
step and the exposed exchange (wall(leg) - wall(attention on the same compute stream), within one process) as median / min / max /
spread (max - min) over the repeats, and the comparisons new against parent and bf16 against fp16 with
    beyond_spread = |difference of medians| > the larger of the two run-to-run spreads.

    python tools/overlap_compare.py DIR --out profiles/bf16_overlap.json [--order "..."] [--what "..."]
"""
import argparse
import glob
import json
import os
import statistics as st

ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--out", required=True)
ap.add_argument("--order", default="parent first, then new, in every repeat")
ap.add_argument("--what", default="")
args = ap.parse_args()

runs = {}
for f in sorted(glob.glob(os.path.join(args.dir, "*.json"))):
    tree, dt, _ = os.path.basename(f)[:-5].split("_")
    runs.setdefault((tree, dt), []).append(json.load(open(f)))


def stat(xs):
    return {"median": round(st.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "spread": round(max(xs) - min(xs), 3),
            "runs": [round(x, 3) for x in xs]}


BASE = {"lane": "attention_on_compute_lane", "default": "attention_on_compute_lane", "layer_op": "attention"}
KEYS = ("wall_ms_per_step", "host_issue_ms_per_step")
table = {}
for (tree, dt), rs in runs.items():
    t = table.setdefault(dt, {}).setdefault(tree, {})
    for leg in rs[0]["legs_ms_per_step"]:
        e = {"wall_ms_per_step": stat([r["legs_ms_per_step"][leg]["wall"] for r in rs]),
             "host_issue_ms_per_step": stat([r["legs_ms_per_step"][leg]["host_issue"] for r in rs])}
        if leg in BASE and BASE[leg] in rs[0]["legs_ms_per_step"]:
            e["exposed_exchange_ms_per_step"] = stat([r["legs_ms_per_step"][leg]["wall"] - r["legs_ms_per_step"][BASE[leg]]["wall"] for r in rs])
        t[leg] = e


def cmp(a, b):
    spread = max(a["spread"], b["spread"])
    return {"a": a["median"], "b": b["median"], "b_minus_a": round(b["median"] - a["median"], 3), "ratio_b_over_a": round(b["median"] / a["median"], 4),
            "run_to_run_spread": spread, "beyond_spread": abs(b["median"] - a["median"]) > spread}


def versus(title, dt_a, tree_a, dt_b, tree_b):
    if dt_a not in table or tree_a not in table[dt_a] or dt_b not in table or tree_b not in table[dt_b]:
        return {}
    return {title: {leg: {k: cmp(table[dt_a][tree_a][leg][k], table[dt_b][tree_b][leg][k]) for k in KEYS} for leg in table[dt_b][tree_b]}}


comparisons = {}
comparisons.update(versus("bf16: this tree (b) against the parent commit (a)", "bf16", "parent", "bf16", "new"))
comparisons.update(versus("fp16: this tree (b) against the parent commit (a)", "fp16", "parent", "fp16", "new"))
comparisons.update(versus("this tree: bf16 (b) against fp16 (a)", "fp16", "new", "bf16", "new"))
comparisons.update(versus("parent commit: bf16 (b) against fp16 (a)", "fp16", "parent", "bf16", "parent"))
one = next(iter(runs.values()))
out = {
    "what": args.what or "tools/overlap_bench.py --dtype {fp16,bf16} in a checkout of the parent commit (with this tree's tools/overlap_bench.py) and in this tree",
    "protocol": f"one GPU call, one process per run, the two checkouts alternating ({args.order}); {len(one)} repeats per tree and dtype; "
                f"--steps {one[0]['steps']} --layers {one[0]['shape']['layers']}; legs in this order: " + ", ".join(one[0]["legs_ms_per_step"])
                + "; aggregated by tools/overlap_compare.py: median / min / max / spread (max - min) over the repeats, exposed exchange = wall(leg) - "
                  "wall(attention on the same compute stream) within one process, beyond_spread = |difference of medians| > the larger of the two spreads",
    "shape": one[0]["shape"],
    "lane": one[0]["lane"],
    "ms_per_step": table,
    "comparisons": comparisons,
}
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
for title, legs in comparisons.items():
    print(title)
    for leg, ks in legs.items():
        print("  %-28s" % leg, "  ".join(f"{k.split('_ms')[0]}: {v['a']} -> {v['b']} ({v['b_minus_a']:+}, spread {v['run_to_run_spread']}, beyond {v['beyond_spread']})"
                                        for k, v in ks.items()))
for dt in table:
    for tree in table[dt]:
        print(dt, tree, "exposed:", {leg: e["exposed_exchange_ms_per_step"]["median"] for leg, e in table[dt][tree].items() if "exposed_exchange_ms_per_step" in e})
