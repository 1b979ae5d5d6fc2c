"""cfx_packet_bytes and cfx_workspace_bytes over a grid of codec arguments, shapes and params: every combination the library answers with a
nonzero packet size, with both values.  Recorded with the library of the commit BEFORE the codec table (cfx_api.hip's codec_table), so that
tests/test_codec_table.py holds the table's size and shape rules to the hand-written switches they replace.  No GPU needed.
usage: python tests/golden/make_golden_codec_sizes.py [path/to/libcfx.so]     (default: the in-tree library)"""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ARGS = list(range(-2, 0x400)) + [0x1001, 0x10001, 0x201]
SHAPES = [(0, 64), (1, 64), (2, 64), (3, 64), (4, 64), (4, 8), (4, 32), (4, 72), (4, 96), (8, 20), (8, 128), (7, 192), (16, 256), (8, 1024)]
PARAMS = [-1, 0, 1, 2, 3, 4, 8, 16, 32, 64, 128, 256]
BATCH = 2
OUT = os.path.join(HERE, "codec_sizes_parent.json")


def sweep(lib):
    """{(arg, N, C, param): (packet bytes, workspace bytes of a batch of 2)} of the nonzero answers, and the number of combinations asked"""
    lib.cfx_packet_bytes.restype = lib.cfx_workspace_bytes.restype = ctypes.c_size_t
    lib.cfx_packet_bytes.argtypes = [ctypes.c_int] * 4
    lib.cfx_workspace_bytes.argtypes = [ctypes.c_int] * 5
    got, total = {}, 0
    for arg, (N, C), p in itertools.product(ARGS, SHAPES, PARAMS):
        total += 1
        pb, wb = lib.cfx_packet_bytes(arg, N, C, p), lib.cfx_workspace_bytes(arg, N, C, p, BATCH)
        if pb or wb:
            got[arg, N, C, p] = (pb, wb)
    return got, total


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(HERE)), "compactfusion_amd", "libcfx.so")
    got, total = sweep(ctypes.CDLL(path))
    assert all(pb for pb, _ in got.values())                    # (no workspace without a packet)
    rows = [list(k) + list(v) for k, v in sorted(got.items())]
    json.dump({"total": total, "batch": BATCH, "columns": ["codec_arg", "N", "C", "param", "packet_bytes", "workspace_bytes"], "rows": rows},
              open(OUT, "w"), separators=(",", ":"))
    print(total, "combinations;", len(rows), "with a packet;", sum(1 for r in rows if r[5]), "with a workspace;",
          len({r[0] for r in rows}), "codec arguments accepted")
