"""The launch skeleton the block-local codecs share (csrc/cfx_local.h: top-k, MXFP4, BINARY_BLOCK) - what can be checked without a GPU:
the gate and hand-over protocol is written once, and the kernels of the three family files compile to the resources they had when every
file carried its own copy (tests/golden/resource_rows_local_parent.json: tools/resource_usage.collect() at the commit before the skeleton,
the rows of cfx_topk.hip, cfx_mx.hip and cfx_bblock.hip)."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "compactfusion_amd", "csrc")
FAMILY = ("cfx_topk.hip", "cfx_mx.hip", "cfx_bblock.hip")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_gate_protocol_is_in_no_family_file():
    for name in FAMILY:
        src = _text(name)
        for word in ("gate_arrive(", "gate_wait<", "p2p_exchange_inline(", "ticket_slot(", "fill_p2p(", "xg->taken", "gate_expect["):
            assert word not in src, (name, word)
        assert "LayerArgs {" not in src and "_PUT(" not in src, name
    shared = _text("cfx_local.h")
    assert shared.count("struct LocalLayerArgs {") == 1
    for word in ("gate_arrive(", "gate_wait<", "p2p_exchange_inline(", "ticket_slot(", "fill_p2p(", "xg->taken", "gate_expect["):
        assert word in shared, word
    # shorter than the three copies were (323 + 295 + 283 lines)
    assert sum(len(_text(n).splitlines()) for n in FAMILY + ("cfx_local.h",)) < 901


def test_an_edit_to_the_shared_header_rebuilds_the_library():
    import inspect
    from compactfusion_amd import build as B
    assert "cfx_local.h" in inspect.getsource(B.needs_build)


@pytest.fixture(scope="module")
def rows():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_usage
    return [k for k in resource_usage.collect() if k["file"] in FAMILY]


def test_every_kernel_compiles_to_no_more_than_before_the_skeleton(rows):
    """SGPR counts are in the fixture and not asserted: they do not bound the occupancy of these kernels."""
    with open(os.path.join(REPO, "tests", "golden", "resource_rows_local_parent.json")) as f:
        parent = {(p["file"], p["demangled"]): p for p in json.load(f)}
    assert len(parent) == 39
    cur = {}
    for k in rows:
        assert (k["file"], k["demangled"]) not in cur, k
        cur[k["file"], k["demangled"]] = k
    assert set(cur) == set(parent), (sorted(set(parent) - set(cur)), sorted(set(cur) - set(parent)))
    for key, p in parent.items():
        k = cur[key]
        assert k.get("scratch", 0) == 0, k
        assert k["vgpr"] + k.get("agpr", 0) <= p["vgpr"] + p["agpr"], (p, k)
        assert k["lds"] <= p["lds"], (p, k)
        assert k["occupancy"] >= p["occupancy"], (p, k)
