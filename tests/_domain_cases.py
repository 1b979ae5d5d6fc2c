"""The shape domain the C-ABI accepts (compactfusion_amd/csrc/cfx_api.hip shape_ok), as test cases built from the dispatch constants -
not at random.  Plain module, shared by tests/test_codec_domain_f64.py (CPU: the oracle against the float64 definition) and
tests/test_gpu_codec_domain.py (GPU: the kernels against the oracle and the definition).

Dispatch rules the shapes cross (each shape says which, beside it):
  C % 128            1-bit / 2-bit layer launch on or off (cfx_absmean.hip gated_one_launch)
  C % 16             min/max layer launch on or off (cfx_minmax.hip)
  CB = ceil(C/512)   <= TICK_MAX_CB (46): in-launch finalize on; 47: off (cfx_api.hip)
  CB*PL*batch        <= MML_MAX_TILES (2048): min/max layer launch on or off
  row tiles          8 / 16 / 32 / 64 / 128 (cfx_i_auto_rows, the layer launches' 32 / 64-row S tiles)
  packet tails       16-byte aligned or not (ld8_tail callers: vector or scalar loads)
"""
CODECS = [("binary", 1, 0), ("int2", 2, 0), ("int4", 3, 0), ("int8", 4, 0),
          ("topk", 5, 1), ("topk", 5, 2), ("topk", 5, 4), ("topk", 5, 8), ("topk", 5, 16)]
CODEC_IDS = [f"{n}{p or ''}" for n, _, p in CODECS]
MAX_BATCH = 16                 # include/cfx.h CFX_MAX_BATCH
TICK_MAX_CB = 46

# (N, C, why).  N: odd, or one past / one short of the row tiles; C: C % 16 == 8, C % 128 != 0 with C % 16 == 0, partial 512-channel
# blocks of 1 / 9 / 17 / 18 / 33 active lanes (8 channels a lane), CB = 46 / 47.
SHAPES = [
    (1, 8, "one row, one lane of one column block"),
    (3, 8, "odd rows, C % 16 == 8"),
    (2, 24, "C % 16 == 8, 3 lanes"),
    (17, 24, "one past the 16-row tile, C % 16 == 8: int8 tails unaligned"),
    (1, 72, "PixArt head dim 72, one row: 9 lanes"),
    (33, 72, "one past 32 rows, C % 16 == 8: int8 tails unaligned"),
    (34, 72, "int4 with N/2 = 17 odd and C % 16 == 8: int4 tails unaligned"),
    (127, 136, "one short of 128 rows, 17 lanes, C % 16 == 8"),
    (130, 136, "int4: N/2 = 65 odd, C % 16 == 8"),
    (129, 144, "PixArt U = 4 shard width; one past 128 rows; C % 128 != 0, C % 16 == 0: 18 lanes"),
    (512, 144, "PixArt 4096/8 rows x 144"),
    (2, 264, "33 lanes, C % 16 == 8"),
    (17, 264, "odd rows, 33 lanes"),
    (513, 192, "SD3 U = 8 shard, one past 512 rows"),
    (129, 384, "FLUX U = 8 shard, odd rows"),
    (3, 520, "two column blocks, the second 1 lane, C % 16 == 8"),
    (66, 520, "int4: N/2 = 33 odd, C % 16 == 8, second block 1 lane"),
    (544, 576, "PixArt U = 2 shard: 544 rows x 576 (C % 128 != 0)"),
    (33, 576, "odd rows x 576"),
    (127, 1160, "C % 16 == 8, third block 17 lanes"),
    (2, 1168, "C % 16 == 0, C % 128 != 0, third block 18 lanes"),
    (129, 1168, "odd rows x 1168"),
    (17, 1920, "C % 128 == 0, 4 blocks (the last 48 lanes)"),
    (2049, 1920, "one past 2048 rows: tall layer form"),
    (2050, 1920, "int4: one past 2048 rows (N/2 odd, C % 16 == 0)"),
    (258, 1160, "int4: N/2 = 129 odd, C % 16 == 8, third block 17 lanes"),
    (514, 576, "int4: N/2 = 257 odd, 514 rows"),
    (126, 23552, "int4: CB = 46, N/2 = 63"),
    (4, 23680, "int4: CB = 47, C % 128 == 0"),
    (18, 8, "int4: N/2 = 9 odd, one lane, C % 16 == 8"),
    (1, 23552, "CB = 46: the last in-launch-finalize width"),
    (3, 23552, "CB = 46, odd rows"),
    (33, 23560, "CB = 47 (finalize off), C % 16 == 8: int8 tails unaligned"),
    (2, 23560, "CB = 47, int4 N/2 = 1 odd: int4 tails unaligned"),
    (17, 23680, "CB = 47, C % 128 == 0"),
    (513, 23680, "CB = 47, one past 512 rows"),
]
# top-k: N*C % 1024 == 0, with 1024-element flat blocks that straddle rows
TOPK_SHAPES = [
    (128, 72, "flat blocks straddle 72-channel rows"),
    (16, 576, "16 x 576: blocks straddle rows"),
    (1, 23552, "one row of 23 blocks, CB = 46"),
    (256, 136, "blocks straddle 136-channel rows (C % 16 == 8)"),
    (128, 8, "8-channel rows: 128 rows a block"),
    (384, 24, "24-channel rows"),
    (512, 144, "PixArt 4096/8 rows x 144"),
    (8, 23680, "CB = 47"),
    (2, 23552, "two rows of 23 blocks"),
]
# the min/max layer's tile count crossing MML_MAX_TILES with a batch of 2 (46 column blocks x 33 row tiles x 2 > 2048)
TILE_CROSSING = (2049, 23552, 2)


def legal(name, N, C, param=0):
    """cfx_api.hip shape_ok"""
    if N < 1 or C < 1 or C % 8:
        return False
    if name == "binary":
        return (N * (C // 8)) % 2 == 0
    if name == "int4":
        return N % 2 == 0
    if name == "topk":
        return (N * C) % 1024 == 0 and param in (1, 2, 4, 8, 16)
    return name in ("int2", "int8")


def shapes_for(name, param=0):
    src = TOPK_SHAPES if name == "topk" else SHAPES
    return [(N, C) for N, C, _ in src if legal(name, N, C, param)]


def tail_offsets(name, N, C, param=0):
    """byte offsets of the packet's sections after the first (include/cfx.h wire layouts)"""
    if name == "binary":
        return [N * C // 8, N * C // 8 + 2 * N]
    if name == "int2":
        return [N * C // 4, N * C // 4 + 2 * N]
    if name == "int4":
        return [N * C // 2, N * C // 2 + 2 * C]
    if name == "int8":
        return [N * C, N * C + 2 * C]
    if name == "topk":
        return [2 * (N * C // param)]
    raise ValueError(name)


def tails_aligned(name, N, C, param=0):
    return all(o % 16 == 0 for o in tail_offsets(name, N, C, param))


# subsets for the costlier paths (every shape here is legal for the codecs that use it; odd / C % 16 == 8 / CB = 47 represented)
FINALIZE_OFF = [(3, 8), (17, 24), (33, 72), (34, 72), (130, 136), (129, 144), (66, 520), (2, 1168), (129, 1168), (2049, 1920),
                (33, 23560), (2, 23560), (513, 23680)]
ROWS_PER_TILE = (16, 32, 64, 128)
BATCH_SHAPES = [(17, 24), (34, 72), (129, 144), (66, 520), (2, 1168), (544, 576), (2, 23560)]
GATED_SHAPES = [(17, 24), (34, 72), (130, 136), (129, 144), (513, 192), (129, 384), (66, 520), (544, 576), (2, 1168), (17, 1920),
                (2049, 1920), (3, 23552), (2, 23560), (17, 23680)]
GRAPH_SHAPES = [(17, 24), (34, 72), (129, 144), (66, 520)]
TOPK_SUBSET = [(128, 72), (256, 136), (16, 576), (8, 23680)]


def subset(name, param, pool):
    if name == "topk":
        pool = TOPK_SUBSET
    return [(N, C) for N, C in pool if legal(name, N, C, param)]
