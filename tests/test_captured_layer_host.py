"""The capturable layer launch of the block-local codecs (include/cfx.h, cfx_set_captured_layer) as far as a machine without a GPU can
check it: the gate protocol's arithmetic in a host model under the sanitizers (tests/capture_gate_model.cpp, its own process), the
setter's return codes and the stats call on a fresh context, configure(captured_layer=...), and the resource rows of the new kernels
(csrc/cfx_capture.hip) against their eager twins.  The GPU side: tests/test_gpu_captured_layer.py."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
CSRC = os.path.join(REPO, "compactfusion_amd", "csrc")
ERR_NULL, ERR_SHAPE = -1, -2
MAX_SLOTS = 4096


def test_gate_model_under_sanitizers(tmp_path):
    """seeded random interleavings of arrivals, entry tickets, polls and give-ups on one slot: every workgroup derives its launch's number,
    the open words are written once per launch with r + 1, nobody passes another launch's gate - and the pool's maximum is the header's"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "capture_gate_model")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           os.path.join(REPO, "tests", "capture_gate_model.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "ok" in r.stdout
    hdr = open(os.path.join(CSRC, "cfx_capture_gate.h")).read()
    assert int(re.search(r"#define CFX_CAP_MAX_SLOTS (\d+)", hdr).group(1)) == MAX_SLOTS


def test_setter_return_codes_and_fresh_stats():
    from compactfusion_amd import _lib
    lib = _lib.load()
    ctx = lib.cfx_create(0)
    assert ctx
    try:
        one, seq, free = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.cfx_captured_layer_stats(ctx, ctypes.byref(one), ctypes.byref(seq), ctypes.byref(free)) == 0
        assert (one.value, seq.value, free.value) == (0, 0, 0)
        assert lib.cfx_captured_layer_stats(ctx, None, None, None) == 0
        assert lib.cfx_set_captured_layer(ctx, 0) == 0                       # the default, again: nothing to do, no HIP call
        assert lib.cfx_set_captured_layer(ctx, -1) == ERR_SHAPE
        assert b"captured layer" in lib.cfx_last_error_string(ctx)
        assert lib.cfx_set_captured_layer(ctx, MAX_SLOTS + 1) == ERR_SHAPE
        assert lib.cfx_captured_layer_release(ctx) == 0                      # no pool: nothing to hand back
        assert lib.cfx_captured_layer_stats(ctx, ctypes.byref(one), ctypes.byref(seq), ctypes.byref(free)) == 0
        assert (one.value, seq.value, free.value) == (0, 0, 0)
        assert lib.cfx_set_captured_layer(None, 0) == ERR_NULL
        assert lib.cfx_captured_layer_stats(None, None, None, None) == ERR_NULL
        assert lib.cfx_captured_layer_release(None) == ERR_NULL
    finally:
        lib.cfx_destroy(ctx)


def test_configure_captured_layer(monkeypatch):
    import compactfusion_amd
    from compactfusion_amd import _lib, config
    assert _lib.load().cfx_set_captured_layer(None, 0) == ERR_NULL           # (the switch this setting drives exists)
    config.reset()
    try:
        monkeypatch.delenv("CFX_CAPTURED_LAYER", raising=False)
        before = compactfusion_amd.configure()
        assert before["captured_layer"] == "0" and config.get("captured_layer") == "0"
        monkeypatch.setenv("CFX_CAPTURED_LAYER", "5")
        assert config.get("captured_layer") == "5"                           # the env var is the default layer ...
        got = compactfusion_amd.configure(captured_layer=8)
        assert got["captured_layer"] == "8" and config.get("captured_layer") == "8"      # ... an explicit configure() overrides it
        monkeypatch.delenv("CFX_CAPTURED_LAYER")
        after = compactfusion_amd.configure(captured_layer=0)
        assert after == before                                               # 0 leaves every other setting as it is
        with pytest.raises(TypeError):
            compactfusion_amd.configure(captured_layers=1)
    finally:
        config.reset()


def test_captured_kernels_resource_rows():
    """one capturable twin per k_*_layer instantiation: no scratch, at most 8 VGPRs above the eager twin, the gate vote's 256 B of LDS.
    The eager rows: tests/golden/resource_rows_codec_table_parent.json, which tests/test_resource_usage.py pins the library's kernels to."""
    import resource_usage as RU
    from compactfusion_amd import _lib, build as B
    assert hasattr(_lib.load(), "cfx_set_captured_layer")
    assert not set(B.CAPTURE_SRC) & set(B.SRC)
    rows = [k for src in B.CAPTURE_SRC for k in RU._one(src)]
    for k, d in zip(rows, RU.demangle([k["name"] for k in rows])):
        k["demangled"] = re.sub(r"^void ", "", re.sub(r"\(.*$", "", d))
    with open(os.path.join(REPO, "tests", "golden", "resource_rows_codec_table_parent.json")) as f:
        eager = {p["demangled"]: p for p in json.load(f) if re.search(r"^k_(topk|mx|bb|i2b|i3b|mxi8)_layer\b", p["demangled"])}
    assert len(eager) == 26, sorted(eager)
    # (cfx_device.h's static k_copy_probe is in every translation unit that includes it; nothing else may be)
    assert all("_layer_cap" in k["demangled"] or k["demangled"] == "k_copy_probe" for k in rows), [k["demangled"] for k in rows]
    cap = {k["demangled"].replace("_layer_cap", "_layer"): k for k in rows if "_layer_cap" in k["demangled"]}
    assert set(cap) == set(eager), (sorted(set(eager) - set(cap)), sorted(set(cap) - set(eager)))
    for name, k in sorted(cap.items()):
        e = eager[name]
        print(f'{k["demangled"]}: vgpr {k["vgpr"]} (eager {e["vgpr"]}) sgpr {k["sgpr"]} scratch {k.get("scratch", 0)} lds {k["lds"]} occupancy {k["occupancy"]}')
        assert k.get("scratch", 0) == 0, k
        assert k.get("agpr", 0) == 0, k
        assert k["vgpr"] <= e["vgpr"] + 8, (k, e)
        assert k["lds"] == 256 and e["lds"] == 256, (k, e)
