"""The codec tables - codec_table in csrc/cfx_api.hip and CODEC_TABLE / NATIVE_CODEC on the Python side - without a GPU: the C table answers
every size question as the hand-written switches before it did (tests/golden/codec_sizes_parent.json, recorded with the library of the
commit before the table), and the two tables name the same codecs with the same bf16 rule."""
import ctypes
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    from compactfusion_amd import _lib
    return _lib.load()


def test_sizes_are_the_parents_over_the_whole_grid(lib):
    spec = importlib.util.spec_from_file_location("make_golden_codec_sizes", os.path.join(HERE, "golden", "make_golden_codec_sizes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.OUT) as f:
        want = json.load(f)
    parent = {tuple(r[:4]): tuple(r[4:]) for r in want["rows"]}
    # (a truncated fixture would pass the zeros for free)
    assert want["total"] == len(gen.ARGS) * len(gen.SHAPES) * len(gen.PARAMS) == 172872 and want["batch"] == gen.BATCH
    assert len(parent) == 1077 and sum(1 for v in parent.values() if v[1]) == 924
    assert len({k[0] for k in parent}) == 17
    got, total = gen.sweep(lib)          # every combination that is nonzero NOW: equal dicts = equal everywhere, the zeros included
    assert total == want["total"]
    assert got == parent, sorted(set(got.items()) ^ set(parent.items()))[:8]


def _accepts(lib, arg):
    return any(lib.cfx_packet_bytes(arg, 8, 128, p) for p in (0, 1, 64))        # (8, 128) is a shape of every codec with one of these params


def test_the_c_table_and_the_python_table_name_the_same_codecs(lib):
    from compactfusion_amd import _lib
    from compactfusion_amd.codecs import CODEC_TABLE, Codec
    assert set(CODEC_TABLE) == set(Codec)
    for cid in range(256):
        row = CODEC_TABLE.get(cid)
        assert _accepts(lib, cid) == (row is not None), cid
        assert _accepts(lib, cid | _lib.ELEM_BF16) == (row is not None and row.bf16), cid


def test_the_exchange_layer_refuses_exactly_the_others(lib):
    """cfx_plan_add_exchange_layer: CFX_ERR_CODEC for what is no codec (or no bf16 codec); anything else for a codec - the op's index on a
    GPU, the failure to create the exchange stream without one"""
    from compactfusion_amd import _lib
    from compactfusion_amd.codecs import CODEC_TABLE
    ctx = lib.cfx_create(0)
    plan = lib.cfx_plan_create(ctx)
    c = (_lib.CompItem * 2)(_lib.CompItem(0x1000, 0x2000, 0x2000, 0x3000), _lib.CompItem(0x4000, 0x5000, 0x5000, 0x6000))
    dd = (_lib.DecompItem * 2)(*[_lib.DecompItem(0x7000, 0x8000, 0x8000)] * 2)
    for cid in range(256):
        row = CODEC_TABLE.get(cid)
        for arg, member in ((cid, row is not None), (cid | _lib.ELEM_BF16, row is not None and row.bf16)):
            param = next((p for p in (0, 1, 64) if lib.cfx_packet_bytes(arg, 8, 128, p)), 0)
            rc = lib.cfx_plan_add_exchange_layer(plan, arg, 8, 128, param, 1, 2, c, 2, dd, None, None, None, 0, None, 0)
            assert (rc == -4) == (not member), (hex(arg), rc)
    lib.cfx_plan_destroy(plan)
    lib.cfx_destroy(ctx)


def test_what_python_derives_from_its_table(monkeypatch):
    from compactfusion_amd import config
    from compactfusion_amd.codecs import CODEC_TABLE, Codec
    from compactfusion_amd.compact import main, slowpath, xlayer
    from compactfusion_amd.compact.utils import COMPACT_COMPRESS_TYPE as T, NATIVE_CODEC
    members = {int(c) for c in Codec}
    for cid in range(256):
        assert xlayer.usable(cid, 2, True) == (cid in members or cid in (101, 102)), cid
    assert slowpath._MAP == {t: c for t, c in NATIVE_CODEC.items() if CODEC_TABLE[c].setting is None}
    assert set(slowpath._MAP) == {T.BINARY, T.INT2, T.INT4, T.INT8, T.SPARSE, T.INT2_MINMAX, T.MXFP4, T.MXINT8}
    # _native at default settings; BINARY (a rank), SPARSE (sparse_ratio) and the low-rank types read the CompactConfig: not here
    for name in ("CFX_BINARY_BLOCK", "CFX_INT2_BLOCK", "CFX_INT3_BLOCK"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(config, "_explicit", {})
    today = {T.INT2: (2, 0), T.INT4: (3, 0), T.INT8: (4, 0), T.INT2_MINMAX: (6, 0), T.MXFP4: (8, 0), T.BINARY_BLOCK: (10, 64),
             T.INT2_BLOCK: (12, 64), T.INT3_BLOCK: (14, 64), T.MXINT8: (16, 0)}
    assert set(today) == set(NATIVE_CODEC) - {T.BINARY, T.SPARSE}
    for t, want in today.items():
        got = main._native(t)
        assert got == want and all(type(v) is int for v in got), (t, got)
    for t in (T.WARMUP, T.IDENTITY, T.LOW_RANK_AWL):
        with pytest.raises(ValueError):
            main._native(t)
    assert main._BF16_TYPES == (T.BINARY, T.INT2, T.BINARY_BLOCK, T.INT2_BLOCK, T.INT3_BLOCK, T.MXINT8)
