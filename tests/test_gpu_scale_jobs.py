"""The scale jobs of the 1-bit and 2-bit layer launches (csrc/cfx_absmean.hip absmean_tagged_jobs) - GPU box only (-m gpu).

A column block's channel-scale job is split over 1, 2 or 4 workgroups, the token-scale job reads a thread's two rows in one round, and the
fp16 scales leave as 16-byte stores where the packet's sections are aligned.  The sums are exact integers, so for every shape, split and
arrival order the packets (bits / codes AND fp16 scales) and every state equal the oracle bit for bit: tests/_scale_jobs.py layer_case,
three back-to-back launches each, own error feedback and looped-back peers, 1-bit and 2-bit, fp16 and bf16, batch 1 and 2.  The product
library chooses the split from the shape (scale_jobs_split: 1 up to P = 9 partials, 2 up to 18, then 4); the developer library can force
it, and tests/scale_jobs_child.py runs the small shapes under every forced split in a process that loaded libcfx_dev.so."""
import os
import subprocess
import sys

import pytest

import _scale_jobs as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("cid", [1, 2], ids=["binary", "int2"])
@pytest.mark.parametrize("N,C", S.ALL_SHAPES)
def test_scale_jobs_match_the_oracle(N, C, cid, bf16, B):
    S.layer_case(cid, bf16, N, C, B)


@pytest.mark.parametrize("cid", [1, 2], ids=["binary", "int2"])
def test_scale_store_paths_are_both_taken(cid):
    """Which store path a shape takes follows from the packet layout alone - V starts 2 N bytes behind the 16-byte aligned U - and the
    alignment shapes must keep pinning both: V per element (N = 2, 130, 132) and in 16-byte stores (544); U with a ragged last group of
    2, 2 and 4 rows and without one.  A layout change that moves a shape to the other path fails here, not silently."""
    got = {N: S.scale_store_paths(cid, N, C) for N, C in S.ALIGNMENT}
    assert got == {2: (False, 2), 130: (False, 2), 132: (False, 4), 544: (True, 0)}
    for N, C in S.ALIGNMENT:
        S.layer_case(cid, False, N, C, 1, seed=7)


@pytest.mark.parametrize("cid", [1, 2], ids=["binary", "int2"])
def test_saturated_partials_through_the_split_jobs(cid):
    """Residuals so large that row and column partials leave the 40-bit tagged words (TAG_SAT, the exact sum beside it: drift 3000 of
    test_layer_launch_partials_beyond_the_tagged_words) at the FLUX shard, where the V job is split and U reads two rows a thread."""
    S.layer_case(cid, False, 544, 3072, 2, drift=3000.0, NP=4, launches=2)


@pytest.mark.parametrize("split", [1, 2, 4])
def test_every_forced_split_on_the_developer_library(split):
    """The split the library chooses never exceeds 1 at the small shapes; the developer library's switch (include/cfx_dev.h
    CFX_DEV_SCALE_SPLIT) forces 1, 2 and 4 there - clamped by the library to max(1, P - 1) and by the reducer bound - in a child process."""
    from compactfusion_amd.build import build_lib
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, CFX_LIBCFX_PATH=build_lib(dev_probes=True))
    r = subprocess.run([sys.executable, os.path.join(here, "scale_jobs_child.py"), str(split)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-3000:])
