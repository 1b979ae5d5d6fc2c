"""Child process of tests/test_gpu_scale_jobs.py::test_every_forced_split_on_the_developer_library: CFX_LIBCFX_PATH points at libcfx_dev.so."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

if __name__ == "__main__":
    import _scale_jobs as S
    from compactfusion_amd import _lib, codecs as K
    split = int(sys.argv[1])
    lib = _lib.load()
    ctx = K.context(0)
    assert lib.cfx_dev_set_probe(ctx, 0x100 + split) == 0
    for N, C in S.SMALL_SHAPES:
        for cid in (1, 2):
            for bf16, B in ((False, 2), (True, 1)):
                S.layer_case(cid, bf16, N, C, B, seed=split)
    assert lib.cfx_dev_set_probe(ctx, 0x100) == 0
    print("ok")
