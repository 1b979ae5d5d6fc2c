"""The capturable layer launch of the block-local codecs (include/cfx.h, cfx_set_captured_layer) as far as a machine without a GPU can
check it: the gate protocol's arithmetic in a host model under the sanitizers (tests/capture_gate_model.cpp, its own process), the
setter's return codes and the stats call on a fresh context, configure(captured_layer=...), and the resource rows of the new kernels
(csrc/cfx_capture.hip) against their eager twins - and against TWINS, the table of tests/_captured_layer.py that the GPU value-domain module
launches them from, with that module's parameter counts, its geometry table and the witnesses' verdict on its seeded inputs.  The GPU side:
tests/test_gpu_captured_layer.py (forms, pool), tests/test_gpu_captured_domain.py (every kernel's value domain, geometry, flags)."""
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


def _cap_names():
    """demangled names of the capturable kernels in the resource rows of build.CAPTURE_SRC"""
    import resource_usage as RU
    from compactfusion_amd import build as B
    rows = [k for src in B.CAPTURE_SRC for k in RU._one(src)]
    names = [re.sub(r"^void ", "", re.sub(r"\(.*$", "", d)) for d in RU.demangle([k["name"] for k in rows])]
    return [n for n in names if "_layer_cap" in n]


def test_twin_table_is_one_to_one_with_the_captured_kernels():
    """tests/_captured_layer.py TWINS - what tests/test_gpu_captured_domain.py launches - against the kernels csrc/cfx_capture.hip compiles
    to: 26 of each, every kernel the twin of exactly one row.  A 27th kernel, or a dropped row, fails here."""
    import _captured_layer as H
    names = _cap_names()
    assert len(names) == len(set(names)) == 26, sorted(names)
    assert len(H.TWINS) == len(set(H.TWINS)) == 26
    want = {("topk", 5, m, False) for m in (1, 2, 4, 8, 16)} | {("mxfp4", 8, 0, False)} | {("mxi8", 16, 0, bf) for bf in (False, True)}
    want |= {(f, cid, B, bf) for f, cid in (("bb", 10), ("i2b", 12), ("i3b", 14)) for B in (32, 64, 128) for bf in (False, True)}
    assert set(H.TWINS) == want
    norm = lambda s: s.replace(" ", "")                      # noqa: E731
    kernels = [norm(t.kernel) for t in H.twins()]
    assert len(set(kernels)) == 26
    assert set(kernels) == {norm(n) for n in names}, (sorted(set(kernels) - {norm(n) for n in names}), sorted({norm(n) for n in names} - set(kernels)))


def test_domain_parameters_cover_every_twin_and_every_case():
    """the parameter list of the GPU value-domain test, counted here: every twin keeps a shape, the parts of a shape's case list are the
    list, and the replays it prescribes are what the case modules say"""
    import _captured_layer as H
    params = H.domain_params()
    assert {t.name for t, *_ in params} == {t.name for t in H.twins()}
    total = 0
    seen = {}
    for t, N, C in params:
        cases = t.cases(N, C)
        assert cases and (t.name, N, C) not in seen
        seen[(t.name, N, C)] = cases
        n = sum(len(t.pairs(c, N, C)) + (1 if t.pairs(c, N, C)[0][0] == 0 else 0) for c in cases)
        assert n == H.prescribed_replays(t, cases, N, C)
        total += n
    print(f"{len(params)} parameters, {total} replays, at most {max(H.prescribed_replays(t, t.cases(N, C), N, C) for t, N, C in params)} in one")
    assert len(params) >= 120 and total >= 4000


def test_geometry_table():
    """the shapes of the GPU geometry tests give the workgroup counts the table names - derived from LOCAL_SU / LOCAL_DU as the host code
    derives them: a changed unit size fails here and does not move the cases -, the ragged ends they are there for, and every twin is legal
    at every one of them"""
    import _captured_layer as H
    hdr = open(os.path.join(CSRC, "cfx_local.h")).read()
    assert (int(re.search(r"#define LOCAL_SU (\d+)", hdr).group(1)), int(re.search(r"#define LOCAL_DU (\d+)", hdr).group(1))) == (4, 8)
    assert (H.LOCAL_SU, H.LOCAL_DU) == (4, 8)
    for t in H.twins():
        for kind, (_, _, n_sw, n_dw) in H.GEOMETRY.items():
            N, C = H.geometry_shape(t, kind)
            assert H.packet_bytes(t, N, C) > 0, (t, kind, N, C)
            assert H.geometry(N, C) == (n_sw, n_dw), (t, kind, N, C, H.geometry(N, C))
            E = N * C
            if kind == "1S-1D":
                assert E <= 1024
            elif kind == "2S-1D":
                assert E == (9216 if t.fam == "topk" else 8448) and E % (256 * 8 * H.LOCAL_SU) != 0
            else:
                assert E == (17408 if t.fam == "topk" else 16512) and E - 256 * 8 * H.LOCAL_DU == (1024 if t.fam == "topk" else 128)
            for c in (t.random_case(), t.adversarial_case()):
                x, st = t.build(c, N, C)
                pkt, nb = t.step(x, st)
                t.witness(x, st, pkt, nb)


@pytest.mark.parametrize("name", ["topk16", "mxfp4", "bb64-fp16", "bb32-bf16", "i2b32-fp16", "i2b64-bf16", "i3b64-fp16", "i3b32-bf16", "mxi8-fp16",
                                  "mxi8-bf16"])
def test_witness_accepts_the_contract_on_the_seeded_batches(name):
    """the inputs the GPU geometry tests draw by seed (tests/_captured_layer.py batch_inputs: no case module's CPU test builds them): the
    family's float64 witness accepts the contract's own output on every one of them, over two rounds"""
    import _captured_layer as H
    assert [t.name for t in H.pick()].count(name) == 1
    t = {t.name: t for t in H.pick()}[name]
    N, C = H.small_shape(t)
    for seed0, n in H.seeded_loads():
        for x, st in H.batch_inputs(t, N, C, n, seed0=seed0):
            for _ in range(2):
                pkt, nb = t.step(x, st)
                t.witness(x, st, pkt, nb)
                st = nb
