"""No kernel of libcfx.so may use scratch memory (register spills).

hipcc's -Rpass-analysis=kernel-resource-usage remarks for every csrc/*.hip, compiled with the product flags (tools/resource_usage.py);
cross-compiled, no GPU needed.  A spill on a default-path kernel is extra HBM traffic nobody planned for ("weak" 2:
k_int2_compress_gated<4> 16 B/lane, k_minmax_layer<int4,8> 12, k_minmax_layer<int8,8> 80).
"""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


@pytest.fixture(scope="module")
def rows():
    import resource_usage
    return resource_usage.collect()


def test_every_kernel_is_seen(rows):
    names = " ".join(k["demangled"] for k in rows)
    for want in ("k_absmean_compress", "k_int2_compress_gated", "k_minmax_layer", "k_topk_layer", "k_lrs", "k_binary_dequant",
                 "k_int2_dequant", "k_minmax_dequant", "k_minmax_quant", "k_attn_merge"):
        assert want in names, want
    assert len(rows) > 60


def test_no_kernel_spills_to_scratch(rows):
    bad = [(k["demangled"], k["scratch"]) for k in rows if k.get("scratch", 0) != 0]
    assert not bad, f"kernels with scratch (bytes per lane): {bad}"


def test_layer_kernels_keep_two_workgroups_a_cu(rows):
    # the one-launch layer forms count on 2 workgroups of 512 threads per CU: <= 128 VGPRs, <= 80 KB of LDS
    for k in rows:
        if any(n in k["demangled"] for n in ("k_absmean_compress", "k_int2_compress_gated", "k_minmax_layer")):
            assert k["vgpr"] + k.get("agpr", 0) <= 128 and k["lds"] <= 80 * 1024, k


def test_one_bit_layer_kernel_leaves_room_for_a_collective_kernel(rows):
    # the collective form of the exchange layer needs RCCL's kernel (256 threads x 280 VGPRs) placed BESIDE a waiting reconstruction
    # workgroup: two waves a SIMD of at most 104 registers leave 512 - 208 = 304 (include/cfx.h, cfx_plan_add_exchange_layer;
    # tests/test_gpu_bench.py::test_bench_with_a_collective_kernel_of_rccl_footprint is the run-time check)
    ks = [k for k in rows if k["demangled"].startswith("k_absmean_compress<true, 4, true")]
    assert ks
    for k in ks:
        assert k["vgpr"] <= 104 or k["demangled"].endswith("true>"), k      # (the <.., true> instantiation carries the developer stamps)


# The min/max family's kernels are templates on RPC, the rows one code row of the packet holds (1 int8, 2 int4, 4 INT2_MINMAX): each
# demangled name of today -> the name it has in the fixtures of earlier commits
MINMAX_FIXTURE_NAME = {
    "k_minmax_quant<1>": "k_int8_quant", "k_minmax_quant<2>": "k_int4_quant", "k_minmax_quant<4>": "k_int2mm_quant",
    "k_minmax_dequant<1>": "k_int8_dequant", "k_minmax_dequant<2>": "k_int4_dequant", "k_minmax_dequant<4>": "k_int2mm_dequant",
    "k_minmax_layer<1, 4>": "k_minmax_layer<false, 4>", "k_minmax_layer<1, 8>": "k_minmax_layer<false, 8>",
    "k_minmax_layer<2, 4>": "k_minmax_layer<true, 4>", "k_minmax_layer<2, 8>": "k_minmax_layer<true, 8>",
    "k_minmax_layer<4, 4>": "k_minmax_layer4<4>", "k_minmax_layer<4, 8>": "k_minmax_layer4<8>",
}
# The kernels whose device code the RPC templates rewrote (the stand-alone quantisers and dequantisers, and the two that call
# minmax_write_scales): they may use fewer registers than the fixture's, never more.  Every other kernel compiles to the fixture's row.
MINMAX_REWRITTEN = {"k_int8_quant", "k_int4_quant", "k_int2mm_quant", "k_int8_dequant", "k_int4_dequant", "k_int2mm_dequant",
                    "k_minmax_finalize", "k_minmax_compress"}


def test_every_kernel_compiles_to_what_it_did_before_the_codec_table(rows):
    """The codec table (csrc/cfx_api.hip codec_table) and the block-local families' shared host tail moved HOST code only:
    tests/golden/resource_rows_codec_table_parent.json is collect() at the commit before them, every kernel of the library.  SGPR counts are
    in the fixture and not asserted: they do not bound the occupancy of these kernels.  Since then the min/max family's kernels became
    templates on RPC (MINMAX_FIXTURE_NAME); the eight of MINMAX_REWRITTEN are held to "no worse", all others to the fixture's row."""
    import json
    with open(os.path.join(REPO, "tests", "golden", "resource_rows_codec_table_parent.json")) as f:
        parent = {(p["file"], p["demangled"]): p for p in json.load(f)}
    assert len(parent) == 192
    assert len(MINMAX_REWRITTEN) == 8 and all(("cfx_minmax.hip", n) in parent for n in MINMAX_REWRITTEN)
    cur = {}
    for k in rows:
        key = k["file"], MINMAX_FIXTURE_NAME.get(k["demangled"], k["demangled"])
        assert key not in cur, k
        cur[key] = k
    assert set(cur) == set(parent), (sorted(set(parent) - set(cur)), sorted(set(cur) - set(parent)))
    for key, p in parent.items():
        k = cur[key]
        if key[1] in MINMAX_REWRITTEN:
            print(f'{k["demangled"]}: vgpr {k["vgpr"]} ({p["vgpr"]}) agpr {k.get("agpr", 0)} ({p.get("agpr", 0)}) occupancy {k["occupancy"]} '
                  f'({p["occupancy"]}) lds {k.get("lds", 0)} ({p.get("lds", 0)}) scratch {k.get("scratch", 0)}')
            assert k["vgpr"] + k.get("agpr", 0) <= p["vgpr"] + p.get("agpr", 0), (p, k)
            assert k["occupancy"] >= p["occupancy"] and k.get("lds", 0) == p.get("lds", 0) and k.get("scratch", 0) == 0, (p, k)
            continue
        for field in ("vgpr", "agpr", "lds", "scratch", "occupancy"):
            assert k.get(field, 0) == p.get(field, 0), (field, p, k)


def test_streaming_stores_of_the_standalone_minmax_kernels_are_non_temporal(tmp_path):
    """Every 16-byte store of k_minmax_quant<RPC> / k_minmax_dequant<RPC> is a state or reconstruction row nobody reads soon: st8nt.  The
    compiler has dropped the flag once - it moves a store out of a loop of one trip (the RPC rows of a code row, int8) as a plain store -
    and the int8 dequantiser ran 8 % slower for it; the assembly says whether it is there."""
    import re
    import subprocess
    from compactfusion_amd import build as B
    src = os.path.join(B.PKG_DIR, "csrc", "cfx_minmax.hip")
    asm = str(tmp_path / "cfx_minmax.s")
    flags = [f for f in B.HIPCC_FLAGS if f not in ("-shared",)]
    r = subprocess.run([B.hipcc_path()] + flags + ["--offload-device-only", "-S", f"-I{B.INC}", f"-I{os.path.join(B.PKG_DIR, 'csrc')}", src, "-o", asm],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(asm).read()
    seen = 0
    for m in re.finditer(r"^(_Z1[46]k_minmax_(?:de)?quantILi[124]E\w+):", text, re.M):
        body = text[m.end():text.index("s_endpgm", m.end())]
        stores = [line.split(";")[0].split() for line in body.splitlines() if "global_store_dwordx4" in line]
        assert stores and all(s[-1] == "nt" for s in stores), (m.group(1), stores)
        seen += 1
    assert seen == 6
