"""One place for the host-side switches of the package: `compactfusion_amd.configure(...)`.

Every setting has a documented default; an environment variable (the round 1-4 switches, kept as a thin default layer so that a
launcher script can set them without touching code) overrides the default, and an explicit `configure()` call overrides both.
Settings are read when they are used, so `configure()` may be called at any time before the layers they affect are (re)built
(`compact_init` / `compact_reset` rebuild them).

    import compactfusion_amd
    compactfusion_amd.configure(exchange="rccl", lane="sticky", lane_exchange_cus=48)

setting                env var                       values / meaning
---------------------  ----------------------------  ---------------------------------------------------------------------------------
exchange               CFX_EXCHANGE                  auto | p2p | rccl | torch - transport of the one-op layer exchange (compact/xlayer.py)
ring_schedule          CFX_RING_SCHEDULE             auto | gather | relay - exchange schedule of compact_fwd (auto: gather on a GPU)
ring_exchange          CFX_RING_EXCHANGE             auto | native | torch - who issues the collective of the multi-launch schedules
ring_exchange_stream   CFX_RING_EXCHANGE_STREAM      auto | xlayer | lane - where a layer's exchange runs: auto = the flag-ordered chain on the
                                                     exchange lane when the caller is on (or is put on) the lane's compute stream, else
                                                     the one-op layer exchange on the caller's stream; xlayer = always the layer op;
                                                     lane = always the chain on the exchange lane
ring_p2p               CFX_RING_P2P                  (unset) | 0 | 1 - 1: the multi-launch chain reads packets in place through IPC mappings too;
                                                     0: no peer-to-peer transport at all (the layer op starts at rccl)
ring_exchange_priority CFX_RING_EXCHANGE_PRIORITY    priority of the unmasked exchange stream: the lane's when the caller is off its compute stream,
                                                     the torch all-gather's (-1)
lane                   CFX_LANE                      auto | sticky | off - how compact_fwd gets onto the exchange lane when the caller is not
                                                     on it already: auto = for the duration of the call (forked from and joined to the
                                                     caller's stream with flag kernels: the model's other kernels keep the caller's stream);
                                                     sticky = the caller's current stream BECOMES the lane's compute stream at the first
                                                     call and stays it (no per-layer hand-over; the rest of the model runs on 224 CUs);
                                                     off = never (the exchange runs as one op on the caller's stream, nothing overlaps)
lane_exchange_cus      CFX_LANE_EXCHANGE_CUS         CUs of the exchange lane (32); the compute lane gets the rest
lowrank_lane           CFX_LOWRANK_LANE              on | off - on: a LOW_RANK / LOW_RANK_Q layer keeps its factor chain (one persistent launch that
                                                     wants the chip) on the compute lane and puts the peers' reconstructions on the exchange lane
                                                     beside the attention blocks; off: the whole layer op on the caller's stream
binary_block           CFX_BINARY_BLOCK              32 | 64 | 128 - block size of COMPACT_COMPRESS_TYPE.BINARY_BLOCK (native codec 10): elements of a row
                                                     that share one fp16 scale (64); read when a layer is (re)built
int2_block             CFX_INT2_BLOCK                32 | 64 | 128 - block size of COMPACT_COMPRESS_TYPE.INT2_BLOCK (native codec 12): elements of a row
                                                     that share one fp16 scale (64); read when a layer is (re)built
int3_block             CFX_INT3_BLOCK                32 | 64 | 128 - block size of COMPACT_COMPRESS_TYPE.INT3_BLOCK (native codec 14): elements of a row
                                                     that share one fp16 scale (64); read when a layer is (re)built
captured_layer         CFX_CAPTURED_LAYER            0 .. 4096 - private gate slots of a context for the block-local codecs' layer launch under hipGraph
                                                     capture (include/cfx.h, cfx_set_captured_layer): 0 (default) = a captured layer call is
                                                     compress ; reconstruct, n = up to n captured layer calls stay ONE launch; applied when a
                                                     context is created and by compact_init / compact_reset
attn_merge             CFX_ATTN_MERGE                chain | once - how a steady layer of compact_fwd merges its W attention blocks: chain (default) = one
                                                     merge launch per block into a running fp32 out / lse (cfx_attn_merge_ex); once = the SDPA
                                                     results are kept and ONE launch merges them after the last block (cfx_attn_merge_many, at
                                                     most 16 blocks), the lane forms' "next peer reconstructed" waits becoming stand-alone
                                                     cfx_flag_wait launches.  The relay schedule and a layer's first (binding) call keep the chain
attention              CFX_ATTENTION                 sdpa | native - who computes a steady layer's attention in compact_fwd: sdpa (default) = the fused SDPA
                                                     op once per K,V block, merged as attn_merge says; native = ONE launch over all W blocks
                                                     where they lie (cfx_attn_fwd_blocks: fp16 / bf16, head dim 64 or 128, at most 16 blocks;
                                                     head dims 72, 80, .. 120 - PixArt's 72, HunyuanDiT's 88 -: cfx_attn_fwd_blocks_hd),
                                                     no per-block results and no merge - attn_merge is ignored; on the lane forms the layer's
                                                     chain is issued first and the launch follows stand-alone cfx_flag_wait launches on every
                                                     peer's flag.  The relay schedule, a layer's first (binding) call, joint tensors (unless
                                                     joint="steady", below), causal, dropout and whatever the launch does not take keep the sdpa path.
                                                     Patch-parallel (patch_gather_fwd): native = ONE launch over [joint?] + the gathered per-rank
                                                     K,V states + [joint?] where they lie, no torch.cat; causal, dropout, a window, more than 16
                                                     blocks and whatever the launch does not take keep the cat + SDPA path
joint                  CFX_JOINT                     general | steady - where a compact_fwd call WITH joint tensors (joint_tensor_key / _value, strategy front or
                                                     rear: the text keys of FLUX, SD3, CogVideoX) runs: general (default) = the general path, one
                                                     block_attention + merge pair per block; steady = the steady layer, once bound, as a call
                                                     without joint tensors does - attention="sdpa": block 0 attends [joint ; own] (front) or block
                                                     W-1 [peer ; joint] (rear), merged as attn_merge says; attention="native": ONE launch over
                                                     [joint, own, peers...] or [own, peers..., joint] with per-block key counts
                                                     (cfx_attn_fwd_blocks_var, at head dims 72 .. 120 cfx_attn_fwd_blocks_hd; W + 1 <= 16 blocks).  The joint K,V are local to every rank: the
                                                     exchange and the K,V states are what the general path leaves, bit for bit
hw_queues              GPU_MAX_HW_QUEUES             hardware queues HIP may give its streams - HIP reads it ONCE when it initialises:
                                                     configure(hw_queues=8) must run before the first CUDA call of the process
"""
from __future__ import annotations

import os
from typing import Any, Dict

_SETTINGS = {
    # name: (env var, default, allowed values or None)
    "exchange": ("CFX_EXCHANGE", "auto", ("auto", "p2p", "rccl", "torch")),
    "ring_schedule": ("CFX_RING_SCHEDULE", "auto", ("auto", "gather", "relay")),
    "ring_exchange": ("CFX_RING_EXCHANGE", "auto", ("auto", "native", "torch")),
    "ring_exchange_stream": ("CFX_RING_EXCHANGE_STREAM", "auto", ("auto", "xlayer", "lane")),
    "ring_p2p": ("CFX_RING_P2P", "", None),
    "ring_exchange_priority": ("CFX_RING_EXCHANGE_PRIORITY", "-1", None),
    "lane": ("CFX_LANE", "auto", ("auto", "sticky", "off")),
    "lane_exchange_cus": ("CFX_LANE_EXCHANGE_CUS", "32", None),
    "lowrank_lane": ("CFX_LOWRANK_LANE", "on", ("on", "off")),
    "binary_block": ("CFX_BINARY_BLOCK", "64", ("32", "64", "128")),
    "int2_block": ("CFX_INT2_BLOCK", "64", ("32", "64", "128")),
    "int3_block": ("CFX_INT3_BLOCK", "64", ("32", "64", "128")),
    "captured_layer": ("CFX_CAPTURED_LAYER", "0", None),
    "attn_merge": ("CFX_ATTN_MERGE", "chain", ("chain", "once")),
    "attention": ("CFX_ATTENTION", "sdpa", ("sdpa", "native")),
    "joint": ("CFX_JOINT", "general", ("general", "steady")),
}
_explicit: Dict[str, str] = {}


def configure(**kw: Any) -> Dict[str, str]:
    """Set host-side switches (see the module docstring); returns the effective settings.  `hw_queues=n` exports GPU_MAX_HW_QUEUES
    for the HIP runtime - it must be called before the process's first CUDA call and raises otherwise."""
    for name, value in kw.items():
        if name == "hw_queues":
            _set_hw_queues(int(value))
            continue
        if name not in _SETTINGS:
            raise TypeError(f"configure() has no setting {name!r}; settings: {', '.join(sorted(_SETTINGS))}, hw_queues")
        allowed = _SETTINGS[name][2]
        value = str(int(value)) if isinstance(value, bool) else str(value)
        if allowed is not None and value not in allowed:
            raise ValueError(f"{name} must be one of {' | '.join(allowed)} (got {value!r})")
        _explicit[name] = value
    return {n: get(n) for n in _SETTINGS}


def get(name: str) -> str:
    env, default, allowed = _SETTINGS[name]
    if name in _explicit:
        return _explicit[name]
    v = os.environ.get(env, default)
    if allowed is not None and v not in allowed:
        raise ValueError(f"{env} must be one of {' | '.join(allowed)} (got {v!r})")
    return v


def reset() -> None:
    """Forget every explicit setting (tests)."""
    _explicit.clear()


def _hip_is_up() -> bool:
    import sys
    torch = sys.modules.get("torch")
    try:
        return torch is not None and torch.cuda.is_initialized()
    except Exception:  # noqa: BLE001
        return True


def _set_hw_queues(n: int) -> None:
    if n < 1:
        raise ValueError("hw_queues must be positive")
    if _hip_is_up() and os.environ.get("GPU_MAX_HW_QUEUES") != str(n):
        raise RuntimeError("configure(hw_queues=...) must run before the first CUDA call of the process: HIP reads GPU_MAX_HW_QUEUES once")
    os.environ["GPU_MAX_HW_QUEUES"] = str(n)
