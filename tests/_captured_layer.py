"""What tests/test_gpu_captured_layer.py (the capturable layer launch's forms and its pool) and tests/test_gpu_captured_domain.py (every one of
the 26 capturable kernels over its family's value domain, launch geometry, flags) share, and what tests/test_captured_layer_host.py reads on the
CPU: TWINS - one row per k_*_layer_cap instantiation of csrc/cfx_capture.hip -, the families' contracts, case lists, comparison rules and
float64 witnesses behind one interface (Twin), and Layer: one layer call on static buffers with the contract's packets and states beside it.
Plain module; nothing here touches the GPU at import."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import _bblock_cases as BBK
import _bblock_f64_check as BBF
import _f64_check as TKF
import _int2block_cases as I2K
import _int2block_f64_check as I2F
import _int3block_cases as I3K
import _int3block_f64_check as I3F
import _mxfp4_cases as MXK
import _mxfp4_f64_check as MXF
import _mxint8_cases as M8K
import _mxint8_f64_check as M8F
import _nonfinite as NF
import _value_cases as V
import bblock_contract as BB
import bf16_contract as BC
import int2block_contract as I2
import int3block_contract as I3
import mxfp4_contract as MX
import mxint8_contract as M8
from oracle import ref_np as R

F16 = np.float16
ELEM_BF16 = 0x100
FLAG_UPDATE_CACHE, FLAG_NO_EF = 1, 2
NB, NP = 2, 4
SHAPES = [(4, 128), (8, 4224)]
LOCAL_SU, LOCAL_DU = 4, 8         # csrc/cfx_local.h: units of 256 threads x 8 elements of an S / a D workgroup
ERR_NULL = -1
MAX_BATCH = 16                    # include/cfx.h CFX_MAX_BATCH; csrc/cfx_capture_gate.h CFX_CAP_MAX_ITEMS ticket lines a slot


def host(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def ref_oracle(*a, **kw):
    from _gpu_codec import oracle
    return oracle(*a, **kw)


def _mx_step(x, st):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pkt, nb = MX.residual_compress(x.view(F16), st.view(F16), True)
    return np.asarray(pkt).view(np.uint16), R.bits(nb)


def _topk_step(x, st):
    N, C = x.shape
    return ref_oracle("topk", x.view(F16), st.view(F16), 8, N, C)


# name -> (codec id, param, bf16, one residual compress on bit patterns: (x, state) -> (packet words, new state bits))
FAMILIES = {"topk8": (5, 8, False, _topk_step), "mxfp4": (MX.CID, 0, False, _mx_step)}
for _B in (32, 128):
    for _bf in (False, True):
        _e = "bf16" if _bf else "fp16"
        FAMILIES[f"bb{_B}-{_e}"] = (BB.CID, _B, _bf, lambda x, st, B=_B, bf=_bf: BB.step(x, st, B, bf))
        FAMILIES[f"i2b{_B}-{_e}"] = (I2.CID, _B, _bf, lambda x, st, B=_B, bf=_bf: I2.step(x, st, B, bf))
        FAMILIES[f"i3b{_B}-{_e}"] = (I3.CID, _B, _bf, lambda x, st, B=_B, bf=_bf: I3.step(x, st, B, bf))
for _bf in (False, True):
    FAMILIES["mxi8-" + ("bf16" if _bf else "fp16")] = (M8.CID, 0, _bf, lambda x, st, bf=_bf: M8.step(x, st, bf))


# ---- the 26 capturable kernels: (family, codec id, param, bf16), one row per k_*_layer_cap instantiation ----------------------------------
TWINS = [("topk", 5, m, False) for m in (1, 2, 4, 8, 16)] + [("mxfp4", MX.CID, 0, False)]
TWINS += [(f, cid, B, bf) for f, cid in (("bb", BB.CID), ("i2b", I2.CID), ("i3b", I3.CID)) for B in (32, 64, 128) for bf in (False, True)]
TWINS += [("mxi8", M8.CID, 0, bf) for bf in (False, True)]
_KERNEL = {"topk": "k_topk_layer_cap", "mxfp4": "k_mx_layer_cap", "bb": "k_bb_layer_cap", "i2b": "k_i2b_layer_cap", "i3b": "k_i3b_layer_cap",
           "mxi8": "k_mxi8_layer_cap"}
_BLOCKED = {"bb": (BB, BBK, BBF), "i2b": (I2, I2K, I2F), "i3b": (I3, I3K, I3F)}


def _nan(bits, bf):
    return (np.asarray(bits) & 0x7FFF) > (0x7F80 if bf else 0x7C00)


def same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, what
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ (first at {int(np.argmax(bad))})"


def same_nan(got, want, what, bf):
    """bits; a NaN where the contract has a NaN (tests/test_gpu_mxfp4.py same, tests/test_gpu_mxint8.py same_state)"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, what
    nan = _nan(want, bf)
    assert _nan(got[nan], bf).all(), f"{what}: not NaN where the contract has NaN"
    same(got[~nan], want[~nan], what)


class Twin:
    """one capturable kernel: its family's contract, cases, comparison rules and witness, all on uint16 bit patterns (N, C)"""

    def __init__(self, fam, cid, param, bf):
        self.fam, self.cid, self.param, self.bf = fam, cid, param, bf
        e = "bf16" if bf else "fp16"
        self.name = {"topk": f"topk{param}", "mxfp4": "mxfp4", "mxi8": f"mxi8-{e}"}.get(fam, f"{fam}{param}-{e}")
        el = "ElemBF16" if bf else "ElemF16"
        self.kernel = _KERNEL[fam] + {"topk": f"<{param}>", "mxfp4": "", "mxi8": f"<{el}>"}.get(fam, f"<{el}, {param}>")
        self.cabi = cid | (ELEM_BF16 if bf else 0)

    def __repr__(self):
        return self.name

    # -- the contract --
    def step(self, x, st, ef=True):
        """one residual compress: (packet words, new state bits); st None: no state"""
        x = np.ascontiguousarray(x).view(np.uint16)
        N, C = x.shape
        st = None if st is None else np.ascontiguousarray(st).view(np.uint16).reshape(N, C)
        f = self.fam
        if f == "topk":
            pkt, nb = ref_oracle("topk", x.view(F16), None if st is None else st.view(F16), self.param, N, C, ef=ef)
        elif f == "mxfp4":
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                pkt, nb = MX.residual_compress(x.view(F16), None if st is None else st.view(F16), ef)
            pkt, nb = np.asarray(pkt).view(np.uint16), R.bits(nb)
        elif f == "mxi8":
            pkt, nb = M8.step(x, st, self.bf, ef)
        else:
            pkt, nb = _BLOCKED[f][0].step(x, st, self.param, self.bf, ef)
        return np.asarray(pkt).view(np.uint16).reshape(-1), np.asarray(nb).view(np.uint16).reshape(N, C)

    def recon(self, pkt, base, N, C):
        """a receiver's reconstruction from a packet (base None: recv itself) -> state bits"""
        base = None if base is None else np.ascontiguousarray(base).view(np.uint16).reshape(N, C)
        f = self.fam
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if f == "topk":
                out = R.bits(R.residual_decompress("topk", pkt, None if base is None else base.view(F16), N, C, self.param))
            elif f == "mxfp4":
                out = R.bits(MX.residual_decompress(pkt, None if base is None else base.view(F16), N, C))
            elif f == "mxi8":
                out = M8.recon(pkt, base, N, C, self.bf)
            else:
                out = _BLOCKED[f][0].recon(pkt, base, N, C, self.param, self.bf)
        return np.asarray(out).view(np.uint16).reshape(N, C)

    # -- the family's case lists (tests/_*_cases.py) --
    def shapes(self):
        """the family's own shapes that this twin's param allows"""
        f = self.fam
        if f == "topk":
            return [s for s in V.TOPK_SHAPES if V.legal("topk", *s, self.param)]
        if f == "mxfp4":
            return list(MXK.SHAPES)
        if f == "mxi8":
            return list(M8K.SHAPES)
        K = _BLOCKED[f][1]
        return [s for s in K.SHAPES if self.param in K.blocks_of(*s)]

    def cases(self, N, C):
        f = self.fam
        if f == "topk":
            return V.cases_for("topk", N, C, self.param)
        if f == "mxfp4":
            return list(MXK.NAMES)
        if f == "mxi8":
            return M8K.cases_for(self.bf)
        return _BLOCKED[f][1].cases_for(self.bf)

    def reps(self, case, N, C):
        f = self.fam
        if f == "topk":
            return V.reps(case, N, C)
        if f == "mxfp4":
            return MXK.reps(case, N, C)
        if f == "mxi8":
            return M8K.reps(case, N, C)
        return _BLOCKED[f][1].reps(case, N, C, self.param)

    def build(self, case, N, C, rep=0, seed=0):
        """(x, state) of a case as bit patterns"""
        f = self.fam
        if f == "topk":
            assert seed == 0
            x, b = V.build(case, "topk", N, C, rep=rep, param=self.param)
        elif f == "mxfp4":
            x, b = MXK.build(case, N, C, rep=rep, seed=seed)
        elif f == "mxi8":
            x, b = M8K.build(case, N, C, self.bf, rep=rep, seed=seed)
        else:
            x, b = _BLOCKED[f][1].build(case, N, C, self.param, self.bf, rep=rep, seed=seed)
        return np.ascontiguousarray(x).view(np.uint16).reshape(N, C), np.ascontiguousarray(b).view(np.uint16).reshape(N, C)

    def pairs(self, case, N, C):
        """(rep of own tensor 0, rep of own tensor 1), one pair per repetition of the case: r and r + 1 as the eager layer tests pair them
        (tests/test_gpu_value_domain.py _run: top-k takes draws 0 and 1; the block-scaled families' test_value_domain_stand_alone_and_layer:
        r and r + 1 modulo the case's reps - there for every other r, here for every r: each repetition is own tensor 0 once)"""
        if self.fam == "topk":
            return [(0, 1)]
        n = self.reps(case, N, C)
        return [(r, (r + 1) % n) for r in range(n)]

    def random_case(self):
        return "ties" if self.fam == "topk" else "random"

    def adversarial_case(self):
        """one case per family whose values sit on the codec's edges (the geometry tests' second input)"""
        return {"topk": "subnormal-and-max", "mxfp4": "edges", "bb": "half-way", "i2b": "half-way", "i3b": "at-thresholds", "mxi8": "ties"}[self.fam]

    def neg_zero_case(self):
        """a case whose recv holds -0 elements - where "recon == recv, bits verbatim" (base NULL) and recv added to a +0 base differ - or
        None: an MXINT8 element has no signed zero, its recv is never -0"""
        return {"topk": "zero-half-blocks", "mxfp4": "zeros", "mxi8": None}.get(self.fam, "subnormals")

    # -- comparison rules and the witness, as the family's eager GPU test has them --
    def same_packet(self, got, want, what):
        if self.fam == "topk":
            NF.same_bits(got, want, what)                         # (tests/_zero_min.py same_packet for every codec but int4)
        else:
            assert np.array_equal(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)), f"{what}: packet bytes differ"

    def same_state(self, got, want, what):
        if self.fam == "topk":
            NF.same_bits(got, want, what)
        elif self.fam in ("mxfp4", "mxi8"):
            same_nan(got, want, what, self.bf)
        else:
            same(got, want, what)

    def witnessed(self, case):
        """whether the eager test runs the float64 witness on this case"""
        if self.fam == "topk":
            return case in V.FINITE
        if self.fam == "mxfp4":
            return case in MXK.FINITE
        return True

    def witness(self, x, before, pkt, state):
        """the family's independent witness on one compress: x, the state before, the packet and the sender's new state"""
        N, C = x.shape
        f = self.fam
        if f == "topk":
            TKF.check("topk", self.param, x.view(F16), before.view(F16), pkt, state.reshape(N, C))
        elif f == "mxfp4":
            MXF.check(x.view(F16), before.view(F16), pkt, state.reshape(N, C))
        elif f == "mxi8":
            M8F.check(x, before, pkt, state.reshape(N, C), bf16=self.bf)
        else:
            _BLOCKED[f][2].check(x, before, pkt, self.param, state.reshape(N, C), bf16=self.bf)


def twins():
    return [Twin(*row) for row in TWINS]


def packet_bytes(t, N, C):
    """cfx_packet_bytes of a twin at a shape (0: the C-ABI refuses the shape)"""
    from compactfusion_amd import _lib
    return _lib.load().cfx_packet_bytes(t.cabi, N, C, t.param)


def domain_params():
    """(twin, N, C) of the value-domain test: the family's own shapes that the twin's param and the C-ABI accept"""
    return [(t, N, C) for t in twins() for N, C in t.shapes() if packet_bytes(t, N, C) > 0]


# launch geometry: kind -> ((N, C) for the block-scaled families, top-k's shape, S workgroups a tensor, D workgroups an item)
GEOMETRY = {"1S-1D": ((1, 64), (128, 8), 1, 1), "2S-1D": ((4, 2112), (128, 72), 2, 1), "3S-2D": ((129, 128), (17, 1024), 3, 2)}


def geometry_shape(t, kind):
    shape, tk, _, _ = GEOMETRY[kind]
    if t.fam == "topk":
        return tk
    if t.param == 128 and kind != "3S-2D":                   # C = 64 and C = 2112 are no multiples of 128: one block; the same E = 8448
        return (1, 128) if kind == "1S-1D" else (33, 256)
    return shape


def prescribed_replays(t, cases, N, C):
    """what the case lists prescribe for a list of cases: one replay per repetition of a case and a second round for its repetition 0"""
    return sum((1 if t.fam == "topk" else t.reps(c, N, C)) + 1 for c in cases)


def pick():
    """one twin per family in each element type it has (block sizes that take C = 192)"""
    names = ["topk16", "mxfp4", "bb64-fp16", "bb32-bf16", "i2b32-fp16", "i2b64-bf16", "i3b64-fp16", "i3b32-bf16", "mxi8-fp16", "mxi8-bf16"]
    by = {t.name: t for t in twins()}
    return [by[n] for n in names]


def small_shape(t):
    return (128, 8) if t.fam == "topk" else (5, 192)


ORDER = [0, 1, 2, 2, 0, 1, 1, 1, 0, 2, 0, 0, 2, 1, 2]        # three layers' replays, interleaved and not in lock step: each five times
BATCH_SEEDS = (500, 700)                                     # the batches of 1 and 16: two loads of up to 16 own tensors
RECOVER_SEEDS = (40, 60, 80)                                 # the recover test: three loads of two layers' two own tensors


def layer_seed(k, done):
    """first seed of layer k's load before its replay number `done` (the three 16-item layers: three own tensors a load)"""
    return 900 + 10 * k + 100 * (done // 2)


def seeded_loads():
    """(first seed, own tensors) of every batch_inputs load whose result goes to a float64 witness on the GPU"""
    out = [(s, MAX_BATCH) for s in BATCH_SEEDS]
    out += [(layer_seed(k, d), 3) for k in range(3) for d in range(0, ORDER.count(k), 2)]
    out += [(s + k, 2) for s in RECOVER_SEEDS for k in range(2)]
    return out


def batch_inputs(t, N, C, n, seed0=500):
    """n (x, state) pairs of random values, one seed an own tensor (tests/test_gpu_bblock.py test_gated_batch_of_16: seed 500 + i; top-k's
    builder has no seed: draw i of its random case)"""
    if t.fam == "topk":
        return [t.build(t.random_case(), N, C, rep=seed0 + i) for i in range(n)]
    return [t.build(t.random_case(), N, C, seed=seed0 + i) for i in range(n)]


def geometry(N, C):
    """(S workgroups a tensor, D workgroups an item) of a layer launch: csrc/cfx_local.h cfx_i_local_layer, csrc/cfx_capture.hip"""
    E = N * C
    return -(-(E // 8) // (256 * LOCAL_SU)), -(-(E // 8) // (256 * LOCAL_DU))


def shape_of(fam, shape):
    return (8, 128) if fam == "topk8" and shape == (4, 128) else shape        # the nearest shape top-k accepts: still 1 S and 1 D workgroup


def dev(u16, bf):
    t = torch.from_numpy(np.ascontiguousarray(u16).view(np.int16))
    return t.view(torch.bfloat16 if bf else torch.float16).cuda()


def _ctx():
    from compactfusion_amd import _lib, codecs as K
    return _lib.load(), K.context(0)


def stats():
    from compactfusion_amd import codecs as K
    s = K.captured_layer_stats(0)
    return s["one_launch"], s["sequence"], s["slots_free"]


def set_pool(n):
    lib, ctx = _ctx()
    assert lib.cfx_set_captured_layer(ctx, n) == 0, lib.cfx_last_error_string(ctx)


@pytest.fixture(autouse=True)
def _clean_pool():
    """every test starts and ends with no pool, no slot handed out and the default switches (its graphs are gone when it returns)"""
    from compactfusion_amd import config
    lib, ctx = _ctx()

    def clean():
        gc.collect()
        torch.cuda.synchronize()
        assert lib.cfx_captured_layer_release(ctx) == 0
        assert lib.cfx_set_captured_layer(ctx, 0) == 0
        assert lib.cfx_set_gated_launch(ctx, 1) == 0
    clean()
    yield
    config.reset()
    clean()


class Layer:
    """one layer call - cfx_compress_batch_gated or the peer-to-peer exchange-layer op (no live peer) - on static buffers: NB own tensors
    with error feedback in place, NP looped-back peers; the oracle's packets and states advance with every step()"""

    def __init__(self, fam, N, C, seed, op="gated"):
        from compactfusion_amd import _lib, codecs as K
        self.lib, self.ctx = _ctx()
        self.cid, self.param, self.bf, self.fn = FAMILIES[fam]
        self.N, self.C, self.op, self.fam = N, C, op, fam
        self.cabi = self.cid | (ELEM_BF16 if self.bf else 0)
        self.rng = np.random.default_rng(seed)
        self.nbytes = K.packet_bytes(self.cabi, N, C, self.param)
        assert self.nbytes > 0, (fam, N, C)
        base = self.fresh()
        self.xin = [dev(b, self.bf) for b in base]
        self.own = [dev(b, self.bf) for b in base]
        self.peer = [dev(base[g % NB], self.bf) for g in range(NP)]
        self.want = [b.copy() for b in base]
        self.wpk = [None] * NB
        slot = (self.nbytes + 255) // 256 * 256
        self.pk = torch.zeros(NB, slot, dtype=torch.uint8, device="cuda")
        self.comp = (_lib.CompItem * NB)(*[_lib.CompItem(self.xin[i].data_ptr(), self.own[i].data_ptr(), self.own[i].data_ptr(),
                                                         self.pk[i].data_ptr()) for i in range(NB)])
        self.gated = (_lib.DecompItem * NP)(*[_lib.DecompItem(self.pk[g % NB].data_ptr(), self.peer[g].data_ptr(), self.peer[g].data_ptr())
                                              for g in range(NP)])
        self.plan = None
        if op == "p2p_layer":
            self.flag = torch.zeros(64, dtype=torch.int32, device="cuda")
            self.plan = self.lib.cfx_plan_create(self.ctx)
            rc = self.lib.cfx_plan_add_exchange_layer_p2p(self.plan, self.cabi, N, C, self.param, _lib.FLAG_UPDATE_CACHE, NB, self.comp, NP,
                                                          self.gated, self.flag.data_ptr(), 0, (ctypes.c_void_p * 1)(), None, 0)
            assert rc >= 0 and self.lib.cfx_plan_finalize(self.plan) == 0, self.lib.cfx_last_error_string(self.ctx)
        self.flags = _lib.FLAG_UPDATE_CACHE

    def fresh(self):
        f = [(self.rng.standard_normal((self.N, self.C)) * 0.5).astype(np.float32) for _ in range(NB)]
        return [BC.f32_to_bf16(a) if self.bf else a.astype(F16).view(np.uint16) for a in f]

    def call(self, sh):
        if self.op == "gated":
            rc = self.lib.cfx_compress_batch_gated(self.ctx, self.cabi, self.N, self.C, self.param, self.flags, NB, self.comp, 0, None, NP,
                                                   self.gated, None, 0, sh)
        else:
            rc = self.lib.cfx_plan_run(self.plan, 0, 1, sh)
        assert rc == 0, self.lib.cfx_last_error_string(self.ctx)

    def step(self):
        """fresh activations into the static buffers; the oracle one step on"""
        xs = self.fresh()
        for i in range(NB):
            self.xin[i].copy_(dev(xs[i], self.bf))
            pkt, nb = self.fn(xs[i].reshape(self.N, self.C), self.want[i].reshape(self.N, self.C))
            self.wpk[i], self.want[i] = np.asarray(pkt).reshape(-1), np.asarray(nb).reshape(self.N, self.C)
        torch.cuda.synchronize()

    def check(self, what):
        torch.cuda.synchronize()
        assert self.lib.cfx_gate_errors(self.ctx) == 0, what
        for i in range(NB):
            if self.wpk[i] is not None:
                same(self.pk[i, :self.nbytes].cpu().numpy().view(np.uint16), self.wpk[i], f"{self.fam} {what}: packet {i}")
            same(host(self.own[i]), self.want[i], f"{self.fam} {what}: sender state {i}")
        for g in range(NP):
            same(host(self.peer[g]), self.want[g % NB], f"{self.fam} {what}: peer state {g}")

    def close(self):
        if self.plan is not None:
            self.lib.cfx_plan_destroy(self.plan)
            self.plan = None


SENTINEL = 0x5A5A                 # what an out-of-place output buffer holds before a launch (a finite fp16 / bf16 value)


class DomainLayer:
    """Layer with everything a test may choose: a Twin, the bit patterns of x and of the own and peer states before a launch (load), nb own
    tensors and npeer reconstruction items (item g reads own tensor g % nb's packet), the flags, in-place or out-of-place outputs, NULL bases
    of the compress items (comp_base False) or of the reconstruction items (peer_base False).  load() sets the inputs, expect() is the
    contract's statement of what one launch on the loaded buffers leaves behind, check() compares - by the family's own rules."""

    def __init__(self, twin, N, C, nb=2, npeer=3, op="gated", flags=FLAG_UPDATE_CACHE, in_place=True, comp_base=True, peer_base=True):
        from compactfusion_amd import _lib, codecs as K
        self.lib, self.ctx = _ctx()
        self.t, self.N, self.C, self.nb, self.npeer, self.op, self.flags = twin, N, C, nb, npeer, op, flags
        self.in_place, self.comp_base, self.peer_base = in_place, comp_base, peer_base
        assert 1 <= nb <= MAX_BATCH and 1 <= npeer <= MAX_BATCH
        bf = twin.bf
        self.nbytes = K.packet_bytes(twin.cabi, N, C, twin.param)
        assert self.nbytes > 0, (twin, N, C)
        zero = np.zeros((N, C), np.uint16)
        fill = np.full((N, C), SENTINEL, np.uint16)
        self.xin = [dev(zero, bf) for _ in range(nb)]
        self.own = [dev(zero, bf) for _ in range(nb)]
        self.peer = [dev(zero, bf) for _ in range(npeer)]
        self.nbuf = self.own if in_place else [dev(fill, bf) for _ in range(nb)]         # new_base of the compress items
        self.rbuf = self.peer if in_place else [dev(fill, bf) for _ in range(npeer)]     # recon of the reconstruction items
        slot = (self.nbytes + 255) // 256 * 256
        self.pk = torch.zeros(nb, slot, dtype=torch.uint8, device="cuda")
        self.comp = (_lib.CompItem * nb)(*[_lib.CompItem(self.xin[i].data_ptr(), self.own[i].data_ptr() if comp_base else None,
                                                         self.nbuf[i].data_ptr(), self.pk[i].data_ptr()) for i in range(nb)])
        self.gated = (_lib.DecompItem * npeer)(*[_lib.DecompItem(self.pk[g % nb].data_ptr(), self.peer[g].data_ptr() if peer_base else None,
                                                                 self.rbuf[g].data_ptr()) for g in range(npeer)])
        self.plan = None
        if op == "p2p_layer":
            self.flag = torch.zeros(64, dtype=torch.int32, device="cuda")
            self.plan = self.lib.cfx_plan_create(self.ctx)
            rc = self.lib.cfx_plan_add_exchange_layer_p2p(self.plan, twin.cabi, N, C, twin.param, flags, nb, self.comp, npeer, self.gated,
                                                          self.flag.data_ptr(), 0, (ctypes.c_void_p * 1)(), None, 0)
            assert rc >= 0 and self.lib.cfx_plan_finalize(self.plan) == 0, self.lib.cfx_last_error_string(self.ctx)
        self.x = self.st = self.pst = None

    def call(self, sh):
        if self.op == "gated":
            rc = self.lib.cfx_compress_batch_gated(self.ctx, self.t.cabi, self.N, self.C, self.t.param, self.flags, self.nb, self.comp, 0, None,
                                                   self.npeer, self.gated, None, 0, sh)
        else:
            rc = self.lib.cfx_plan_run(self.plan, 0, 1, sh)
        assert rc == 0, self.lib.cfx_last_error_string(self.ctx)

    def load(self, ins, peers=None):
        """ins: nb (x, state) bit patterns; peers: the npeer peer states (default: peer g holds own tensor g % nb's state)"""
        assert len(ins) == self.nb
        bf = self.t.bf
        self.x = [np.ascontiguousarray(x).copy() for x, _ in ins]
        self.st = [np.ascontiguousarray(b).copy() for _, b in ins]
        self.pst = [np.ascontiguousarray(p).copy() for p in peers] if peers is not None else [self.st[g % self.nb].copy() for g in range(self.npeer)]
        for i in range(self.nb):
            self.xin[i].copy_(dev(self.x[i], bf))
            self.own[i].copy_(dev(self.st[i], bf))
        for g in range(self.npeer):
            self.peer[g].copy_(dev(self.pst[g], bf))
        if not self.in_place:
            fill = dev(np.full((self.N, self.C), SENTINEL, np.uint16), bf)
            for t in self.nbuf + self.rbuf:
                t.copy_(fill)
        torch.cuda.synchronize()

    def new_x(self, xs):
        """other activations over the states as they are"""
        self.x = [np.ascontiguousarray(x).copy() for x in xs]
        for i in range(self.nb):
            self.xin[i].copy_(dev(self.x[i], self.t.bf))
        torch.cuda.synchronize()

    def expect(self):
        """one launch on the model: -> (packets, new_base outputs or None where nothing is written, recon outputs, states before); the model's
        own and peer states move on as the buffers do"""
        N, C, t = self.N, self.C, self.t
        upd, ef = bool(self.flags & FLAG_UPDATE_CACHE), not (self.flags & FLAG_NO_EF)
        before = [s.copy() for s in self.st]
        pk, nbo = [], []
        for i in range(self.nb):
            p, nb = t.step(self.x[i], self.st[i] if self.comp_base else None, ef)
            pk.append(p)
            nbo.append(nb if upd else None)
        rec = [t.recon(pk[g % self.nb], self.pst[g] if self.peer_base else None, N, C) for g in range(self.npeer)]
        if self.in_place:
            self.st = [nbo[i] if upd else self.st[i] for i in range(self.nb)]
            self.pst = rec
        return pk, nbo, rec, before

    def check(self, want, what, witness=False):
        """the buffers after one launch against expect()'s statement; witness: the family's float64 witness on every own tensor"""
        pk, nbo, rec, before = want
        t = self.t
        torch.cuda.synchronize()
        assert self.lib.cfx_gate_errors(self.ctx) == 0, f"{what}: gate errors"
        for i in range(self.nb):
            got = self.pk[i, :self.nbytes].cpu().numpy().view(np.uint16)
            t.same_packet(got, pk[i], f"{what}: packet {i}")
            if nbo[i] is not None:
                t.same_state(host(self.nbuf[i]), nbo[i], f"{what}: sender state {i}")
                if witness:
                    t.witness(self.x[i], before[i], got, host(self.nbuf[i]))
            elif not self.in_place:
                same(host(self.nbuf[i]), np.full(self.N * self.C, SENTINEL, np.uint16), f"{what}: new_base {i} written without UPDATE_CACHE")
            if nbo[i] is None or not self.in_place:
                same(host(self.own[i]), before[i], f"{what}: own state {i} must be untouched")
            same(host(self.xin[i]), self.x[i], f"{what}: x {i} must be untouched")
        for g in range(self.npeer):
            t.same_state(host(self.rbuf[g]), rec[g], f"{what}: peer state {g}")
            if not self.in_place:
                same(host(self.peer[g]), self.pst[g], f"{what}: peer base {g} must be untouched")

    def close(self):
        if self.plan is not None:
            self.lib.cfx_plan_destroy(self.plan)
            self.plan = None


def capture(side, fn):
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            fn(side.cuda_stream)
    torch.cuda.synchronize()
    return graph


def eager(side, layer, what):
    layer.step()
    with torch.cuda.stream(side):
        layer.call(side.cuda_stream)
    layer.check(what)


# ---- the HIP runtime torch has loaded, through ctypes: capture on a raw stream handle, the nodes of the captured graph -----------------
class Hip:
    def __init__(self):
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        assert path, "the HIP runtime is not loaded"
        h = self.h = ctypes.CDLL(path)
        V, P = ctypes.c_void_p, ctypes.POINTER
        for name, args in (("hipStreamBeginCapture", [V, ctypes.c_int]), ("hipStreamEndCapture", [V, P(V)]),
                           ("hipGraphGetNodes", [V, P(V), P(ctypes.c_size_t)]), ("hipGraphNodeGetType", [V, P(ctypes.c_int)]),
                           ("hipGraphInstantiate", [P(V), V, P(V), ctypes.c_char_p, ctypes.c_size_t]), ("hipGraphLaunch", [V, V]),
                           ("hipGraphExecDestroy", [V]), ("hipGraphDestroy", [V]), ("hipStreamSynchronize", [V])):
            fn = getattr(h, name)
            fn.argtypes, fn.restype = args, ctypes.c_int

    def capture(self, sh, fn):
        """(graph, executable graph, types of its nodes) of what fn enqueues on the stream with handle sh"""
        V = ctypes.c_void_p
        torch.cuda.synchronize()
        assert self.h.hipStreamBeginCapture(V(sh), 2) == 0                    # hipStreamCaptureModeRelaxed
        try:
            fn(sh)
        finally:
            g = V()
            rc = self.h.hipStreamEndCapture(V(sh), ctypes.byref(g))
        assert rc == 0 and g.value
        n = ctypes.c_size_t(0)
        assert self.h.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
        nodes = (V * max(1, n.value))()
        assert self.h.hipGraphGetNodes(g, nodes, ctypes.byref(n)) == 0
        types = []
        for i in range(n.value):
            t = ctypes.c_int(-1)
            assert self.h.hipGraphNodeGetType(V(nodes[i]), ctypes.byref(t)) == 0
            types.append(t.value)
        ex = V()
        assert self.h.hipGraphInstantiate(ctypes.byref(ex), g, None, None, 0) == 0 and ex.value
        return g, ex, types

    def launch(self, ex, sh):
        assert self.h.hipGraphLaunch(ex, ctypes.c_void_p(sh)) == 0
        assert self.h.hipStreamSynchronize(ctypes.c_void_p(sh)) == 0

    def destroy(self, g, ex):
        self.h.hipGraphExecDestroy(ex)
        self.h.hipGraphDestroy(g)


KERNEL_NODE = 0          # hipGraphNodeTypeKernel
