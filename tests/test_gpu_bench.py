"""bench.py end to end on one GPU (-m gpu): the contract line at N = 1 (the collective in the headline schedule, roofline + cpu_baseline
objects) and the N > 1 plumbing - plans laid out for several live ranks, both exchange patterns, the uncompressed exchange issued
natively in both patterns, the xgmi object - over tests/fake_rccl in loop-back mode (`--emulate-live`).  Reduced layer count: the
judged workload is the default command line, this only checks that every leg runs and the keys are there."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _fake():
    sys.path.insert(0, os.path.join(HERE, "fake_rccl"))
    try:
        import build as fake_build
        return fake_build.build()
    finally:
        sys.path.pop(0)
        sys.modules.pop("build", None)


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--full", "--layers", "6", "--steps", "3", "--warmup", "1", "--long-steps", "3",
                        "--cpu-seconds", "0.5", "--overlap-steps", "0", *args], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, "stdout carries ONE line, the JSON (library chatter - RCCL's version banner - belongs on stderr): %r" % lines[:-1]
    return json.loads(lines[-1])


def test_plain_run_times_the_steps_and_dumps_what_the_last_step_left(tmp_path):
    """Without --full the line carries the headline alone (no CPU baseline, no secondary leg), and --dump-outputs writes the states the last
    timed step left as float32 within 64 MB: the same arguments twice give the same files, bit for bit."""
    import numpy as np

    def plain(out):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--layers", "6", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=REPO)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 1, lines[:-1]
        return json.loads(lines[-1])
    d = plain(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["exchange_issued_by"] == "p2p" and d["launches_per_layer"] == 1
    assert "cpu_baseline" not in d and d["long_run"] is None and d["two_launches_per_layer"] is None and "plugin_path" not in d
    plain(tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["own_state.npy", "peer_reconstructions.npy"] and sorted(os.listdir(tmp_path / "b")) == names
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all() and np.array_equal(a, b), n


@pytest.mark.parametrize("warmup", [1, 4])
def test_bench_falls_back_when_the_collective_cannot_be_placed(warmup):
    """a collective kernel that needs an EMPTY CU (CFX_FAKE_RCCL_FAT=2) never runs beside the waiting layer launch: the validation step times
    out (300 ms gates), every rank switches to two launches per layer, the line says so and the states are still consistent.  (8 live
    ranks: 14 peer tensors' reconstruction tiles wait on every CU; with 2 live ranks only the one peer's tiles wait - the own
    error-feedback update takes its scales from the launch's tagged words since round 5 - and most CUs are empty)
    warmup 4 (round 6): the launch of the SECOND step is refused on a context whose first step timed out (CFX_ERR_GATE) - that used to end
    the bench with a RuntimeError for every --warmup > 1, i.e. for the driver's own command line; now the first step is validated by itself
    and a refused step waits for the validation instead of raising (runner.guarded_step)."""
    os.environ["CFX_FAKE_RCCL_FAT"] = "2"
    try:
        d = _bench("--emulate-live", "8", "--rccl-lib", _fake(), "--no-cpu-baseline", "--no-raw-baseline", "--layers", "3", "--warmup", str(warmup))
    finally:
        os.environ.pop("CFX_FAKE_RCCL_FAT", None)
    assert d["launches_per_layer"] == 2 and "failed validation" in d["schedule_fallback"] and "gate" in d["schedule_fallback"]


def test_bench_with_a_collective_kernel_of_rccl_footprint():
    """CFX_FAKE_RCCL_FAT=1: the loop-back collective as a kernel of 256 threads x 280 VGPRs (rcclGenericKernel on gfx950) - placed beside
    the waiting reconstruction group (which leaves 32 workgroup slots free), no fall-back"""
    os.environ["CFX_FAKE_RCCL_FAT"] = "1"
    try:
        d = _bench("--emulate-live", "8", "--rccl-lib", _fake(), "--no-cpu-baseline", "--no-raw-baseline")
    finally:
        os.environ.pop("CFX_FAKE_RCCL_FAT", None)
    assert d["launches_per_layer"] == 1 and d["schedule_fallback"] is None


def test_bench_collective_in_the_path_still_selectable():
    d = _bench("--p2p", "off", "--no-cpu-baseline")
    assert "ncclAllGather" in d["schedule"] and "flag-wait kernel" in d["schedule"] and d["exchange_issued_by"] == "native" and d["launches_per_layer"] == 1


def test_bench_two_launch_schedule_still_selectable():
    d = _bench("--own-ef", "ride", "--no-cpu-baseline")
    assert "ncclAllGather" in d["schedule"] and d["launches_per_layer"] == 2 and "k_binary_dequant" in d["roofline"]["kernel"]


def test_bench_default_line_has_the_collective_in_its_schedule():
    d = _bench()
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["vs_baseline"] is None and "workload" in d["config"]
    # N = 1: the layer is ONE codec launch gated on the collective's arrival (exchange-layer op); the two-launch form, the flag relay and
    # the CU-partitioned configuration ride along as secondary legs
    assert "NO collective" in d["schedule"] and "cfx_plan_add_exchange_layer_p2p" in d["schedule"] and d["exchange_issued_by"] == "p2p" and d["launches_per_layer"] == 1
    for k in ("collective_in_the_path", "two_launches_per_layer", "flag_relay_no_communicator", "with_cu_partition"):
        assert d[k]["ms_per_step"] > 0, k
    assert "k_absmean_compress<bits,gated>" in d["roofline"]["kernel"]
    assert d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] < 1 and d["roofline"]["peak"] == 8000.0
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1 and "parity_spot_check" in d["cpu_baseline"]
    assert d["loopback_one_launch_per_layer"]["ms_per_step"] > 0 and d["pure_exchange_upper_bound"]["ms_per_step"] > 0


@pytest.mark.parametrize("live,pattern", [(2, "allgather"), (3, "relay"), (8, "allgather")])
def test_bench_n_gt_1_plumbing_over_the_loopback_library(live, pattern):
    d = _bench("--emulate-live", str(live), "--rccl-lib", _fake(), "--exchange-pattern", pattern, "--no-cpu-baseline")
    assert d["n_gpus"] == 1 and d["exchange_pattern"] == pattern and d["exchange_issued_by"] == "native"
    # all-gather pattern: the exchange-layer op at every N (first step validated, no fall-back needed here); the relay pattern keeps two launches
    assert d["launches_per_layer"] == (1 if pattern == "allgather" else 2) and d["schedule_fallback"] is None
    x = d["xgmi"]
    assert x["pattern"] == pattern and x["links"] == (1 if pattern == "relay" else min(live - 1, 7))
    assert set(x["compressed"]) == {"allgather", "relay"} and set(x["raw"]) == {"allgather", "relay"}
    for leg in list(x["compressed"].values()) + list(x["raw"].values()):
        # loop-back device copies: a rate, no fraction of a LINK roofline (a device copy may exceed the link peak; VERDICT round 4, task 8)
        assert leg["ms_per_step"] > 0 and leg["achieved"] > 0 and leg["unit"] == "GB/s" and "frac" not in leg and leg["loopback_device_copy"]
    assert x["wire_bytes_per_gpu_per_step"] == (live - 1) * 2 * 6 * d["config"]["packet_bytes"]
    assert x["raw_bytes_per_gpu_per_step"] == (live - 1) * 2 * 6 * d["config"]["raw_bytes"]
    assert "no Python-issued collective" in x["issued_by"]
    assert d["raw_exchange_ms_per_step"].keys() == {"allgather", "relay"} and d["speedup_vs_raw_allgather"] > 0


def test_bench_two_rank_processes_exchange_peer_to_peer():
    """N = 2 as the driver launches it (torch.distributed.run, one process per rank) - on ONE GPU here (--same-gpu --backend gloo; RCCL refuses
    two ranks on a device, so there is no collective library at all): the packets stay in each process's IPC-shared buffer, the other
    process's reconstruction workgroups read them in place, one published word per rank and layer (cfx_plan_add_exchange_layer_p2p).  The
    bench validates its first step (gate timeouts, state consistency across the ranks) and checks the states again at the end."""
    env = dict(os.environ)
    env.setdefault("GPU_MAX_HW_QUEUES", "8")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29613", os.path.join(REPO, "bench.py"), "--full", "--gpus", "2", "--same-gpu", "--backend", "gloo", "--layers", "6",
                        "--steps", "4", "--warmup", "1", "--long-steps", "4", "--overlap-steps", "0", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=600, cwd=REPO, env=env)
    assert r.returncode == 0, r.stderr[-2500:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 2 and d["exchange_issued_by"] == "p2p" and d["launches_per_layer"] == 1 and d["schedule_fallback"] is None
    assert "NO collective" in d["schedule"] and d["scaling"] == "weak"
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, "under torch.distributed.run too stdout carries ONE line, rank 0's JSON: %r" % lines[:-1]
    # the rank processes share one GPU: a rate, but no fraction of a LINK roofline - no link carried a byte
    assert d["xgmi"]["same_gpu"] and "frac" not in d["xgmi"] and "frac" not in d["xgmi"]["compressed"]["allgather"]


@pytest.mark.parametrize("poison_step", [1, 3])
def test_bench_poisoned_peer_state_falls_back_instead_of_dying(poison_step):
    """N = 2 (two rank processes on one GPU, no collective library): after step 1 (warm-up) / step 3 (inside the timed region) rank 0
    corrupts one reconstructed state - what a stale cache line in a reader's L2 would leave from the SECOND use of an address on.  The
    validation after the warm-up steps / after the timed region trips on every rank together, the run continues in-process on the next
    schedule (here torch.distributed per layer: RCCL refuses two ranks on a device), exits 0 and says which check tripped."""
    env = dict(os.environ)
    env.setdefault("GPU_MAX_HW_QUEUES", "4")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(29620 + poison_step), os.path.join(REPO, "bench.py"), "--full", "--gpus", "2", "--same-gpu", "--backend", "gloo",
                        "--layers", "6", "--steps", "4", "--warmup", "2", "--long-steps", "4", "--overlap-steps", "0", "--no-cpu-baseline",
                        "--poison-after-step", str(poison_step)],
                       capture_output=True, text=True, timeout=600, cwd=REPO, env=env)
    assert r.returncode == 0, r.stderr[-2500:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    fb = d["schedule_fallback"]
    assert d["n_gpus"] == 2 and d["exchange_issued_by"] == "torch" and d["launches_per_layer"] == 2, d
    assert fb and "peer-to-peer" in fb and "differs from its owner" in fb and ("after the warm-up steps" if poison_step == 1 else "after the timed region") in fb, fb
