"""Build libcfx.so (the HIP kernels + C-ABI) in-tree with hipcc for gfx950.

The shared object is git-ignored but travels to the GPU box with the repo snapshot.
`python -m compactfusion_amd.build` or `__graft_entry__.build()` calls this.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG_DIR)
SRC = [os.path.join(PKG_DIR, "csrc", f) for f in ("cfx_api.hip", "cfx_absmean.hip", "cfx_minmax.hip", "cfx_topk.hip", "cfx_mx.hip", "cfx_bblock.hip", "cfx_i2block.hip", "cfx_i3block.hip", "cfx_mxint8.hip", "cfx_plan.hip", "cfx_lowrank.hip", "cfx_lrgram.hip", "cfx_lrslab.hip")]
# The capturable layer launches of the block-local codecs (include/cfx.h, cfx_set_captured_layer): compiled into the same libcfx.so, listed
# BESIDE SRC - tests/test_resource_usage.py pins the kernels of SRC to what they were before this file existed.
CAPTURE_SRC = [os.path.join(PKG_DIR, "csrc", "cfx_capture.hip")]
# The one-launch merge of all of a layer's attention blocks (include/cfx.h, cfx_attn_merge_many): a list of its own for the same reason -
# tests/test_captured_layer_host.py pins the kernels of CAPTURE_SRC too.
MERGE_SRC = [os.path.join(PKG_DIR, "csrc", "cfx_merge.hip")]
# The native attention forward over all of a layer's K,V blocks (include/cfx.h, cfx_attn_fwd_blocks): again a list of its own -
# tests/test_attn_merge_many_f64.py pins the kernels of MERGE_SRC.
ATTN_SRC = [os.path.join(PKG_DIR, "csrc", "cfx_attn.hip")]
# The same forward for K,V blocks of unequal length (include/cfx.h, cfx_attn_fwd_blocks_var): a list of its own once more -
# tests/test_attn_fwd_f64.py pins the kernels of ATTN_SRC.
ATTN_VAR_SRC = [os.path.join(PKG_DIR, "csrc", "cfx_attn_var.hip")]
# ... and for the head dims between 64 and 128 (include/cfx.h, cfx_attn_fwd_blocks_hd): a list of its own for the same reason -
# tests/test_attn_var_f64.py pins the kernels of ATTN_VAR_SRC.
ATTN_HD_SRC = [os.path.join(PKG_DIR, "csrc", "cfx_attn_hd.hip")]
INC = os.path.join(REPO, "include")
LIB = os.path.join(PKG_DIR, "libcfx.so")
LIB_DEV = os.path.join(PKG_DIR, "libcfx_dev.so")      # the same sources with -DCFX_DEV_PROBES (include/cfx_dev.h): tools and one test only
ARCH = "gfx950"

HIPCC_FLAGS = [
    f"--offload-arch={ARCH}", "-O3", "-std=c++17",
    "-ffp-contract=off",          # one rounding per reference op: no fma contraction of u*v + base
    "-fPIC", "-shared",
]


def hipcc_path() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: cannot build libcfx.so")


def needs_build(lib: str = LIB) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    deps = SRC + CAPTURE_SRC + MERGE_SRC + ATTN_SRC + ATTN_VAR_SRC + ATTN_HD_SRC + [os.path.join(INC, "cfx.h"), os.path.join(INC, "cfx_dev.h"), os.path.join(PKG_DIR, "csrc", "cfx_internal.h"),
                  os.path.join(PKG_DIR, "csrc", "cfx_lr.h"), os.path.join(PKG_DIR, "csrc", "cfx_device.h"), os.path.join(PKG_DIR, "csrc", "cfx_host.h"),
                  os.path.join(PKG_DIR, "csrc", "cfx_local.h"), os.path.join(PKG_DIR, "csrc", "cfx_bscale.h")]
    deps += [os.path.join(PKG_DIR, "csrc", h) for h in ("cfx_capture_gate.h", "cfx_topk.h", "cfx_mx.h", "cfx_bblock.h", "cfx_i2block.h", "cfx_i3block.h", "cfx_mxint8.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build_lib(force: bool = False, verbose: bool = False, dev_probes: bool = False) -> str:
    """The product library libcfx.so - or, dev_probes, the DEVELOPER library libcfx_dev.so: the same sources with -DCFX_DEV_PROBES
    (per-workgroup phase stamps in the kernels, the launch-tag test hook, early exits of the compress kernel: include/cfx_dev.h).  The
    product library has none of that compiled in and exports none of those symbols."""
    lib = LIB_DEV if dev_probes else LIB
    if not force and not needs_build(lib):
        return lib
    cmd = [hipcc_path()] + HIPCC_FLAGS + (["-DCFX_DEV_PROBES"] if dev_probes else []) + [f"-I{INC}", f"-I{os.path.join(PKG_DIR, 'csrc')}"] + SRC + CAPTURE_SRC + MERGE_SRC + ATTN_SRC + ATTN_VAR_SRC + ATTN_HD_SRC + ["-o", lib + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stdout + r.stderr)
    os.replace(lib + ".tmp", lib)
    return lib


def build_both(force: bool = False) -> tuple:
    """Product and developer library side by side (two hipcc processes)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(2) as ex:
        a, b = ex.submit(build_lib, force, False, False), ex.submit(build_lib, force, False, True)
        return a.result(), b.result()


if __name__ == "__main__":
    print(build_lib(force="--force" in sys.argv or "--dev-probes" in sys.argv, verbose=True, dev_probes="--dev-probes" in sys.argv))
