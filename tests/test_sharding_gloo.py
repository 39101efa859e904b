"""N > 1 path on CPU: world_size-2 gloo processes exercise the sharding logic bench.py uses on GPUs
(contiguous element ranges, one twiddle-block broadcast, no data-path collective).  The compute inside
each rank is the oracle here (no GPU in this container); on the GPU box the same ranges feed the HIP path."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from stark_rings_amd.sharding import shard_range


def test_shard_range_partitions_exactly():
    for batch in (0, 1, 7, 8, 9, 16384, 65536, 100003):
        for world in (1, 2, 3, 4, 8):
            got = [shard_range(batch, world, r) for r in range(world)]
            assert got[0][0] == 0
            for (f0, c0), (f1, _) in zip(got, got[1:]):
                assert f0 + c0 == f1
            assert got[-1][0] + got[-1][1] == batch
            counts = [c for _, c in got]
            assert max(counts) - min(counts) <= 1
    with pytest.raises(ValueError):
        shard_range(10, 2, 2)


def test_multi_gpu_selection_widens_with_the_device_count():
    """what the GPU suite does on a box with more than one device is decided by two small functions -- checked here on
    the CPU for every device count, so that the branches a one-GPU box never takes are at least exercised as logic."""
    from stark_rings_amd.sharding import group_device_ids, rehearsal_backend

    assert group_device_ids(0) == [0, 0] and group_device_ids(1) == [0, 0]      # the one-GPU form: two contexts on device 0
    assert group_device_ids(2) == [0, 1] and group_device_ids(4) == [0, 1, 2, 3]
    assert group_device_ids(8) == list(range(8)) and group_device_ids(16) == list(range(8))
    for n in range(2, 17):
        ids = group_device_ids(n)
        assert len(set(ids)) == len(ids) == min(n, 8)                            # distinct devices: the peer copy crosses xGMI
    assert rehearsal_backend(0) == ("gloo", 2) and rehearsal_backend(1) == ("gloo", 2)
    assert rehearsal_backend(2) == ("nccl", 2) and rehearsal_backend(8) == ("nccl", 2)


def _worker(rank, world, port, k, batch, tmp):
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import oracle_lib as O
    from stark_rings_amd.sharding import broadcast_block, init_process_group, shard_range

    init_process_group("gloo", rank, world)
    try:
        # 1. the one collective: rank 0's table bytes reach every rank intact
        ref = np.frombuffer(np.random.default_rng(1234).bytes(1 << 16), dtype=np.uint8).copy()
        block = torch.from_numpy(ref.copy() if rank == 0 else np.full_like(ref, 0xAB))
        broadcast_block(block, src=0)
        assert np.array_equal(block.numpy(), ref), "broadcast mismatch on rank %d" % rank
        # 2. independent shards: each rank multiplies only its element range; nothing is exchanged
        F = O.GOLDILOCKS
        d = 1 << k
        first, count = shard_range(batch, world, rank)
        a = O.fill_uniform(F, 0x5EED0001, first * d, count * d)
        b = O.fill_uniform(F, 0x5EED0002, first * d, count * d)
        c = O.pow2_ring_mul(F, a, b, k, count, 1) if count else np.zeros(0, dtype=np.uint64)
        np.save(os.path.join(tmp, "shard%d.npy" % rank), c)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,batch", [(2, 5), (2, 8)])
def test_two_rank_shards_reassemble_to_the_unsharded_result(tmp_path, world, batch):
    import socket

    import oracle_lib as O

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    k = 8
    mp.spawn(_worker, args=(world, port, k, batch, str(tmp_path)), nprocs=world, join=True)
    parts = [np.load(os.path.join(str(tmp_path), "shard%d.npy" % r)) for r in range(world)]
    got = np.concatenate(parts)
    F = O.GOLDILOCKS
    a = O.fill_uniform(F, 0x5EED0001, 0, batch << k)
    b = O.fill_uniform(F, 0x5EED0002, 0, batch << k)
    assert np.array_equal(got, O.pow2_ring_mul(F, a, b, k, batch, 2))


@pytest.mark.gpu
def test_bench_launches_its_own_ranks_and_checks_every_shard():
    """`python bench.py --gpus 2` with no torchrun environment: bench.py starts the two ranks itself (a child torch.distributed.run,
    before the parent touches HIP), both ranks share the one GPU of the test box over gloo, each checks a sample of ITS shard
    against the oracle, and rank 0 prints one JSON line for the whole job."""
    import json
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--backend", "gloo", "--batch", "6", "--steps", "2",
           "--warmup", "1", "--parity-sample", "6", "--cpu-seconds", "0.5"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 12
    assert d["multi_gpu"]["ranks_seen"] == 2 and d["multi_gpu"]["data_path_collectives"] == 0
    assert d["multi_gpu"]["twiddle_broadcast_bytes"] > 0
    assert "6 sampled elements per rank (2 ranks)" in d["parity"]
    assert d["value"] > 0


@pytest.mark.gpu
def test_bench_ranks_over_rccl_when_the_box_has_two_gpus():
    """The sibling that widens itself: on a box with two or more visible GPUs the same self-launched two-rank run goes
    over `nccl` (= RCCL) with one rank per DISTINCT device -- the first multi-rank RCCL broadcast of the twiddle block, a real
    inter-GPU transfer -- each rank checking its shard against the oracle.  On the one-GPU box of the round's driver the selection
    (stark_rings_amd.sharding.rehearsal_backend; unit-tested on the CPU above) says gloo, which the test above already runs: skipped.
    The ranks are CHILDREN of a child (bench.py's own torch.distributed.run), nothing re-execs a process that holds the GPU."""
    import json
    import subprocess

    from stark_rings_amd.sharding import rehearsal_backend

    backend, ranks = rehearsal_backend(torch.cuda.device_count())   # device_count() does not initialise HIP on this image
    if backend != "nccl":
        pytest.skip("one visible GPU: the gloo rehearsal above is the form of this test that applies")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", str(ranks), "--backend", "nccl", "--batch", "300", "--steps", "2",
           "--warmup", "1", "--parity-sample", "6", "--cpu-seconds", "0.5"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == ranks and d["multi_gpu"]["backend"].startswith("nccl") and d["multi_gpu"]["ranks_seen"] == ranks
    assert d["multi_gpu"]["devices_visible"] >= 2 and d["multi_gpu"]["data_path_collectives"] == 0
    assert "6 sampled elements per rank (%d ranks)" % ranks in d["parity"]


@pytest.mark.gpu
def test_sharded_path_at_config_4_degree_every_shard_sampled():
    """BASELINE config 4's degree (D = 2^20, 42 MB of tables to broadcast) through the sharded path before an 8-GPU
    node ever runs it: `bench.py --gpus 2 --workload goldilocks_d1048576_b8192 --batch 16` launches its two ranks itself (children,
    never a re-exec of a process that touched the GPU), rank 0 broadcasts the table block over gloo, each rank multiplies ITS 16
    elements of degree 2^20 (two lane chunks of 8) and checks every one of them against the oracle."""
    import json
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--backend", "gloo", "--workload", "goldilocks_d1048576_b8192",
           "--batch", "16", "--steps", "2", "--warmup", "1", "--parity-sample", "16", "--cpu-seconds", "0.5"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 32 and "1048576" in d["config"]["workload"]
    assert d["multi_gpu"]["ranks_seen"] == 2 and d["multi_gpu"]["data_path_collectives"] == 0
    assert d["multi_gpu"]["twiddle_broadcast_bytes"] > 40 << 20
    assert "16 sampled elements per rank (2 ranks)" in d["parity"]
    assert d["value"] > 0


@pytest.mark.gpu
def test_bench_single_rank_reports_the_plan_the_library_chose():
    """`python bench.py` on a batch of several chunks: bench.py has no probe of its own -- the library settled the plan inside
    sr_ctx_reserve_scratch (sr_plan.lanes = 0) and config.plan quotes its measurement; the sampled elements are bit-exact against the
    oracle; with --calibrate and the lanes in use the line carries the overlap note and the labelled one-stream calibration."""
    import json
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SR_LANES")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--batch", "1100", "--steps", "3", "--warmup", "1", "--parity-sample", "5",
           "--cpu-seconds", "0.5", "--calibrate"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["config"]["global_batch"] == 1100   # eight lane chunks and more: the probe runs
    assert "5 sampled elements per rank" in d["parity"]
    plan = d["config"]["plan"]
    assert plan.startswith("library default (sr_plan.lanes = 0, auto): ") and "its probe took" in plan
    roof = d["roofline"]
    assert 0 < roof["frac"] < 1 and 0 < roof["whole_step_frac"] < 1
    # every kernel tag of the step carries its own per-launch fraction; the reported one is the subject kernel's
    assert set(roof["by_kernel"]) == {"fwd_cols", "rows", "inv_cols"}
    assert abs(roof["by_kernel"][roof["kernel"]]["frac"] - roof["frac_events"]) < 1e-9
    assert roof["launches_per_step_by_kernel"]["fwd_cols"] == roof["launches_per_step_by_kernel"]["rows"]  # both operands: one launch
    assert "multi_gpu" not in d
    # the line itself says why the whole step is where it is -- the reported fraction is the lower of the event-sampled
    # and the rocprof-replayed figure, the events bracket a sparse sample (the profiled steps run like the timed ones), clock and
    # power were sampled during the timed steps, and the whole-step VALU issue fraction is there whenever profiles/ holds PMC
    # counters of this very build
    assert roof["frac"] <= roof["frac_events"] + 1e-12 and roof["limiter"]
    assert roof["events"]["bracketed"].startswith("every 7") and roof["events"]["sampled_launches"] > 0
    assert abs(roof["events"]["profiled_step_ms"] / roof["events"]["timed_step_ms"] - 1) < 0.15
    if "clock_power" in d:   # (a box without readable amdgpu hwmon files has none)
        assert 400 < d["clock_power"]["sclk_mhz"] < 2600 and 100 < d["clock_power"]["socket_w"] < 1500 and d["clock_power"]["samples"] >= 1
    if "replayed" in roof.get("rocprof_source", "") or "dropped: " in roof["traffic_source"]:
        import bench

        pj = [os.path.join(ROOT, "profiles", r, "pmc_goldilocks_d65536_b16384.json") for r in sorted(os.listdir(os.path.join(ROOT, "profiles")))]
        pj = [q for q in pj if os.path.exists(q)][-1]
        if json.load(open(pj)).get("source_sha256") == bench.source_hash():
            ws = d["integer_valu"]["whole_step"]
            assert 0.3 < ws["frac_at_nominal_2400_mhz"] < 1.0 and ws["valu_wave_instructions_per_step"] > 0
            if "clock_power" in d:
                assert 0.3 < ws["frac"] < 1.05 and ws["issue_floor_ms_at_sampled_clock"] < roof["events"]["timed_step_ms"] * 1.05
    if "two lanes --" in plan and "overlap" in roof:
        assert roof["overlap"]["internal_streams"] == 2 and roof["overlap"]["factor"] > 1.2
        assert roof["single_stream"]["frac"] > roof["frac"]  # the same kernel alone is faster per launch than beside the other lane


@pytest.mark.gpu
def test_bench_force_dist_executes_the_rccl_path_on_one_gpu():
    """`python bench.py --force-dist`: the N > 1 code path on the one GPU of the box -- a ONE-rank `nccl` (= RCCL) process group is
    initialised before anything else touches the card, the twiddle block is broadcast through the DeviceBytes view of the library's own
    allocation and adopted (twiddles_updated), the rank count, the step times and the parity verdict are all-reduced on DEVICE tensors,
    and the product computed with the adopted tables is bit-exact against the oracle.  No re-exec: bench.py runs as a plain child."""
    import json
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SR_LANES")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--force-dist", "--batch", "600", "--steps", "2", "--warmup", "1",
           "--parity-sample", "4", "--cpu-seconds", "0.5"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    mg = d["multi_gpu"]
    assert mg["backend"] == "nccl (RCCL)" and mg["ranks_seen"] == 1 and mg["data_path_collectives"] == 0
    assert mg["twiddle_broadcast_bytes"] > 2 << 20      # [tw | itw | tuned tables] of D = 2^16
    assert mg["rank_ms_per_step"]["min"] <= mg["rank_ms_per_step"]["max"]
    assert any("parity" in c for c in mg["collectives_run"])
    assert d["n_gpus"] == 1 and "4 sampled elements per rank (1 ranks)" in d["parity"]
    assert d["value"] > 0
