"""The low-rank RECEIVER and the factor quantiser, element by element against float64 - GPU box only (-m gpu).

The deterministic stages of the low-rank family - k_lr_decode (VALU), k_lr_decode_mfma, k_lr_dq4 and k_lr_q4 (csrc/cfx_lowrank.hip) - have
an output that their input defines.  Host-built packets (tests/_lr_cases.py; LOW_RANK_Q packets by the pinned int4 oracle, never by a
kernel of the library) go through the public entry codecs.lr_decompress_batch, and the result goes against the float64 witness
tests/_lr_f64_check.py: lo <= out <= hi element by element, most elements pinned to one value (tests/test_lr_f64_host.py holds how many).
Every call: `out` lies between canary rows that must come back untouched, packet and base come back bit-identical, no gate error, and
the launches are PROVED by the kernel ids of cfx_profile_read - one decode launch (22), for LOW_RANK_Q one factor-dequant launch (12) in
front of it.

  * every instantiation: decode mode 1 (VALU) and 2 (MFMA) forced with cfx_set_lr_decode, ranks 2 .. 32 (RP = 8, 16, 32; r == RP and
    r != RP), both wire forms, the smallest shapes that take every branch; mode 0 once per rank (the automatic choice);
  * the multi-pass MFMA walk (64 and 128 rows a workgroup: the row0 loop runs more than once, V fragments held across passes) - the
    product reaches it at (4096, 1152) x 14 peers, and the shapes here are the smallest that do, by the host rule restated in
    tests/_lr_cases.py rows_per_wg;
  * batch 1, 3, 16 of distinct packets, with and without a base in one batch; recon aliased to base (compact/main.py reconstructs in place);
  * sender == receiver under every decode mode: lr_compress_batch's new state equals lr_decompress_batch of its packet bit for bit, and
    passes the witness given the packet.  The slab-resident chain fuses the update in the VALU form's summation order: after
    cfx_set_lr_decode(ctx, 2) it has to leave the update to the MFMA form the receiver then runs (csrc/cfx_lrslab.hip cfx_i_lrs_factors);
  * k_lr_q4 against the int4 contract bit for bit, in a child process on the developer library (tests/lr_q4_child.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _gpu_codec as GC
import _lr_cases as LC
import _lr_f64_check as W

pytestmark = pytest.mark.gpu

CANARY = 0x7E00
GUARD = 4                          # canary rows in front of and behind `out`
KID_DQ4, KID_DECODE = 12, 22


def _api():
    from compactfusion_amd import _lib, codecs as K
    return _lib.load(), K, K.context(0)


@pytest.fixture(autouse=True)
def _switches_back():
    lib, K, ctx = _api()
    yield
    assert lib.cfx_set_lr_decode(ctx, 0) == 0 and lib.cfx_set_lr_chain(ctx, 0) == 0


def dev16(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int16).copy()).cuda().view(torch.float16)


def decode(quant, N, C, r, items, inplace=False):
    """lr_decompress_batch of items [(packet words, base fp16 or None)] -> out bits per item, with everything a call must leave alone checked"""
    lib, K, ctx = _api()
    B = len(items)
    pk = [dev16(p) for p, _ in items]
    bufs = [torch.full((N + 2 * GUARD, C), CANARY, dtype=torch.int16, device="cuda").view(torch.float16) for _ in range(B)]
    recs = [b[GUARD:GUARD + N] for b in bufs]
    if inplace:
        assert all(b is not None for _, b in items)
        for rec, (_, b) in zip(recs, items):
            rec.copy_(dev16(np.ascontiguousarray(b).view(np.uint16)).view(N, C))
        bases = recs
    else:
        bases = [None if b is None else dev16(np.ascontiguousarray(b).view(np.uint16)).view(N, C) for _, b in items]
    ids = GC._profile(ctx, lib, lambda: K.lr_decompress_batch(quant, pk, bases, recs, N, C, r))
    assert ids == ([KID_DQ4, KID_DECODE] if quant else [KID_DECODE]), ids
    assert lib.cfx_gate_errors(ctx) == 0
    outs = []
    for i, (p, b) in enumerate(items):
        assert np.array_equal(GC.host(pk[i]).reshape(-1), np.ascontiguousarray(p).view(np.uint16).reshape(-1)), f"item {i}: the packet changed"
        if b is not None and not inplace:
            assert np.array_equal(GC.host(bases[i]), np.ascontiguousarray(b).view(np.uint16)), f"item {i}: the base changed"
        h = GC.host(bufs[i])
        assert (h[:GUARD] == CANARY).all() and (h[GUARD + N:] == CANARY).all(), f"item {i}: wrote outside out's {N} rows"
        outs.append(h[GUARD:GUARD + N])
    return outs


def witness(quant, N, C, r, pkt, U, V, base, out, what, exact=False):
    share = W.check_q(pkt, N, C, r, base, out, what) if quant else W.check(U, V, base, out, what)
    if exact:
        assert share == 1.0, (what, share)
    return share


def case_items(quant, N, C, r):
    """a batch of distinct packets: every case with its base, and `random` / `integers` draws without one"""
    spec = [(n, LC.random_rep(quant, N, C, r, True) if n == "random" else 0, True) for n in LC.NAMES]
    spec += [("random", LC.random_rep(quant, N, C, r, False), False), ("integers", 1, False)]
    out = []
    for name, rep, withbase in spec:
        U, V, base = LC.build(name, N, C, r, rep, quant)
        out.append((name, U, V, base if withbase else None, LC.packet(quant, U, V)))
    return out


def run_items(quant, N, C, r, its, what, inplace=False):
    outs = decode(quant, N, C, r, [(p, b) for _, _, _, b, p in its], inplace)
    for (name, U, V, base, pkt), out in zip(its, outs):
        witness(quant, N, C, r, pkt, U, V, base, out, f"{what} {name} ({N}, {C}) r={r} {'Q' if quant else 'plain'}", exact=name in LC.EXACT)


FORMS = [(False, r) for r in LC.RANKS] + [(True, r) for r in LC.RANKS_Q]


@pytest.mark.parametrize("quant,r", FORMS, ids=[f"{'q' if q else 'plain'}-r{r}" for q, r in FORMS])
@pytest.mark.parametrize("mode", [1, 2], ids=["valu", "mfma"])
def test_every_instantiation_against_the_witness(mode, quant, r):
    lib, K, ctx = _api()
    assert lib.cfx_set_lr_decode(ctx, mode) == 0
    for N in (LC.NS_Q if quant else LC.NS):
        for C in LC.CS:
            run_items(quant, N, C, r, case_items(quant, N, C, r), f"mode {mode}")


@pytest.mark.parametrize("quant,r", FORMS, ids=[f"{'q' if q else 'plain'}-r{r}" for q, r in FORMS])
def test_the_automatic_choice_against_the_witness(quant, r):
    """mode 0: the VALU form up to rank 16, the MFMA form above - whichever it is, the same contract"""
    lib, K, ctx = _api()
    assert lib.cfx_set_lr_decode(ctx, 0) == 0
    N = (LC.NS_Q if quant else LC.NS)[-1]
    for C in LC.CS:
        run_items(quant, N, C, r, case_items(quant, N, C, r), "mode 0")


WALKS = [(q, N, C, rows, r) for q, N, C, rows in LC.WALK for r in LC.WALK_RANKS[q]]


@pytest.mark.parametrize("name", LC.WALK_CASES)
@pytest.mark.parametrize("quant,N,C,rows,r", WALKS, ids=[f"{'q' if q else 'plain'}-{N}x{C}-rows{rows}-r{r}" for q, N, C, rows, r in WALKS])
def test_multi_pass_mfma_walk(quant, N, C, rows, r, name):
    """cfx_i_lr_decode_launch lets a workgroup of the MFMA form walk 128 or 64 rows where ceil(C / 512) * ceil(N / rows) * batch >= 768
    (LC.rows_per_wg restates it: whoever changes the rule re-derives these shapes).  (129, 11784) x 16: 24 * 2 * 16 = 768, one group of
    four passes and one of a single row; (70, 11784) x 16: 384 at 128, 768 at 64 - two passes and a six-row group; (37, 1032) x 16 stays
    at 32.  LOW_RANK_Q needs an even N: 130 and 38."""
    lib, K, ctx = _api()
    B = LC.WALK_BATCH
    assert LC.rows_per_wg(N, C, B) == rows
    assert lib.cfx_set_lr_decode(ctx, 2) == 0
    its = []
    for i in range(B):
        rep = i % 4 if name == "random" else i
        U, V, base = LC.build(name, N, C, r, rep, quant)
        its.append((name, U, V, None if i % 4 == 3 else base, LC.packet(quant, U, V)))
    outs = decode(quant, N, C, r, [(p, b) for _, _, _, b, p in its])
    for i, ((_, U, V, base, pkt), out) in enumerate(zip(its, outs)):             # the witness item by item: its float64 arrays stay small
        witness(quant, N, C, r, pkt, U, V, base, out, f"walk {name} item {i} ({N}, {C}) r={r} rows={rows}", exact=name in LC.EXACT)


@pytest.mark.parametrize("quant", [False, True], ids=["plain", "q"])
@pytest.mark.parametrize("r", LC.BATCH_RANKS)
@pytest.mark.parametrize("B", [1, 3, 16])
def test_batches_of_distinct_packets(B, r, quant):
    N, C = LC.BATCH_SHAPE
    its = []
    for i in range(B):
        U, V, base = LC.build("random", N, C, r, i, quant)
        its.append(("random", U, V, None if i % 3 == 1 else base, LC.packet(quant, U, V)))
    run_items(quant, N, C, r, its, f"batch {B}")


@pytest.mark.parametrize("quant", [False, True], ids=["plain", "q"])
@pytest.mark.parametrize("r", LC.BATCH_RANKS)
@pytest.mark.parametrize("mode", [1, 2], ids=["valu", "mfma"])
def test_recon_aliased_to_base(mode, r, quant):
    """compact/main.py reconstructs peers in place: lr_decompress_batch(quant, a, b, b, ...)"""
    lib, K, ctx = _api()
    assert lib.cfx_set_lr_decode(ctx, mode) == 0
    N, C = LC.BATCH_SHAPE
    its = []
    for name, rep in (("random", 0), ("random", 2), ("integers", 0), ("one-hot", 0), ("zero-rows", 0)):
        U, V, base = LC.build(name, N, C, r, rep, quant)
        its.append((name, U, V, base, LC.packet(quant, U, V)))
    run_items(quant, N, C, r, its, f"in place, mode {mode}", inplace=True)


@pytest.mark.parametrize("quant", [False, True], ids=["plain", "q"])
@pytest.mark.parametrize("r", [8, 16])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["auto", "valu", "mfma"])
def test_sender_state_equals_receiver_under_every_decode_mode(mode, r, quant):
    """lr_compress_batch(update_cache, ef) then lr_decompress_batch of its packet, cfx_set_lr_decode set before both: the sender's new
    state and the receiver's reconstruction are the same bits, and the reconstruction is what the packet defines.  Items without a base
    among them: there the state is fp16(U V) itself, and two summation orders show wherever their fp32 sums straddle an fp16 boundary."""
    lib, K, ctx = _api()
    assert lib.cfx_set_lr_decode(ctx, mode) == 0
    N, C = LC.SENDER_SHAPE
    B, rp = 8, K.lr_rank_pad(r)
    rng = np.random.default_rng(1000 * mode + 10 * r + int(quant))
    xs, bases, q0s = [], [], []
    for i in range(B):
        b = rng.standard_normal((N, C)).astype(np.float16)
        xs.append((b.astype(np.float32) + 0.1 * rng.standard_normal((N, C)).astype(np.float32)).astype(np.float16) if i % 2 == 0
                  else rng.standard_normal((N, C)).astype(np.float16))
        bases.append(b if i % 2 == 0 else None)
        q0 = np.zeros((C, rp), np.float32)
        q0[:, :r] = rng.standard_normal((C, r)).astype(np.float32)
        q0s.append(torch.from_numpy(q0).cuda())
    xd = [GC.dev(x) for x in xs]
    bd = [None if b is None else GC.dev(b) for b in bases]
    nb = [torch.full((N, C), CANARY, dtype=torch.int16, device="cuda").view(torch.float16) for _ in range(B)]
    rec = [torch.full((N, C), CANARY, dtype=torch.int16, device="cuda").view(torch.float16) for _ in range(B)]
    pk = [torch.zeros(K.lr_packet_halves(quant, N, C, r), dtype=torch.float16, device="cuda") for _ in range(B)]
    K.lr_compress_batch(quant, xd, bd, nb, pk, q0s, N, C, r, update_cache=True, ef=True)
    K.lr_decompress_batch(quant, pk, bd, rec, N, C, r)
    torch.cuda.synchronize()
    assert lib.cfx_gate_errors(ctx) == 0
    diff = [int((GC.host(nb[i]) != GC.host(rec[i])).sum()) for i in range(B)]
    print(f"sender != receiver elements per item (mode {mode}, r {r}, {'Q' if quant else 'plain'}): {diff}")
    for i in range(B):
        p = GC.host(pk[i]).reshape(-1)
        U, V = (None, None) if quant else (p[:N * r].reshape(N, r), p[N * r:].reshape(r, C))
        witness(quant, N, C, r, p, U, V, bases[i], GC.host(rec[i]).reshape(N, C), f"receiver item {i} mode {mode} r={r}")
    assert diff == [0] * B, f"sender state differs from the receiver's reconstruction: {diff} elements per item"


def test_factor_quantiser_against_the_int4_contract():
    """k_lr_q4 alone (cfx_dev_lr_q4, developer library) in a fresh child process: tests/lr_q4_child.py"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k != "CFX_LIBCFX_PATH"}
    r = subprocess.run([sys.executable, os.path.join(here, "lr_q4_child.py")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
