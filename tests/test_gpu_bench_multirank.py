"""Rehearsal of bench.py's N > 1 control flow on the 1-GPU box: two ranks share device 0, the
per-shard top-k travel over gloo (VROD_BENCH_BACKEND=gloo), and the merged result of the last
batch must equal a single-device search of the whole corpus.  Every N > 1 line of a `--full` run must
carry the metric's recall / exactness fields WITHOUT any further switch (VROD_BENCH_VERIFY unset).
(The measured multi-GPU runs use
RCCL, one GPU per rank; this checks sharding, id offsets, the packed exchange, the merge and the
pipelined loop, not performance.)
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_multi_gpu_fields(out):
    """BASELINE.json's metric is QPS + recall@10 vs the CPU reference at 1/2/4/8 GPUs: the three fields of an N > 1 line"""
    assert out["verify_merged_equals_single_device"] is True
    assert "hipcc" in out["library"]          # vrod_version(): the compiler that built the device code
    assert out["recall_at_10"] == 1.0
    assert out["bit_exact_vs_oracle_on_sample"] is True
    assert "oracle_sample" in out and "parity" in out


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_bench_two_ranks_on_one_device(world):
    env = dict(os.environ, VROD_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("VROD_BENCH_VERIFY", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(29560 + world), os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "3", "--warmup", "1",
           "--rows", "300001", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().split("\n") if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == world and out["steps"] == 3
    assert_multi_gpu_fields(out)
    assert out["exactness"]["certificate_fallback_queries"] == 0


@pytest.mark.gpu
def test_bench_plain_gpus_2_launches_its_own_ranks():
    """`python bench.py --gpus 2` with NO launcher in the command (the way the driver starts the
    1-GPU run): the parent starts the ranks itself, relays ONE JSON line and the ranks' exit code."""
    env = dict(os.environ, VROD_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("VROD_BENCH_VERIFY", None)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(v, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--rows", "300001", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().split("\n") if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1
    assert_multi_gpu_fields(out)
    pr = out["per_rank"]
    assert pr["backend"] == "gloo" and pr["rccl_ranks"] == 0     # rehearsal backend: not an RCCL measurement
    assert len(pr["scan_ms_per_step"]["all"]) == 2
    assert 0 < pr["scan_ms_per_step"]["min"] <= pr["scan_ms_per_step"]["max"]
    assert pr["allgather_merge_ms_per_step"]["max"] > 0 and pr["wall_ms_per_step"]["max"] > 0


def test_bench_world_size_mismatch_is_an_error():
    """WORLD_SIZE=4 with --gpus 8 must not silently report n_gpus=4 (checked before torch is imported)."""
    env = dict(os.environ, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=4" in r.stderr and r.stdout.strip() == ""


@pytest.mark.gpu
@pytest.mark.parametrize("rccl", ["1", "0"])
def test_bench_inprocess_two_shards_one_handle(rccl):
    """`bench.py --inprocess --gpus 2`: one process, one multi-device handle, the exchange inside the
    library (RCCL all-gather; VROD_RCCL=0: peer copies).  On the 1-GPU box both shards sit on device 0."""
    env = dict(os.environ, VROD_BENCH_DEVICES="0,0", VROD_RCCL=rccl, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("VROD_BENCH_VERIFY", None)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(v, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--inprocess", "--gpus", "2", "--steps", "4", "--warmup", "1", "--rows", "400001",
           "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().split("\n") if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2
    assert_multi_gpu_fields(out)
    assert ("RCCL all-gather" in out["config"]["parallelism"]) == (rccl == "1")
    # what each shard's device spent (vrod_index_shard_stats)
    assert [d["shard"] for d in out["per_device"]] == [0, 1] and all(d["device"] == 0 and d["scan_ms_per_step"] > 0 for d in out["per_device"])


def test_bench_rejects_zero_steps():
    """--steps sets the number of timed steps: none to time is an error (before torch is imported)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0", "--warmup", "0"],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr and r.stdout.strip() == ""


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_timed_batch(tmp_path):
    """A plain single-GPU run times its steps and nothing else (the oracle, the probes are --full items); --dump-outputs
    writes the last timed batch's ids and scores, which equal a search of that batch (query rows of the last step)."""
    import numpy as np
    import torch
    import vrod_amd as va
    steps, warmup, rows, nq, k = 3, 2, 300001, 1024, 10
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--rows", str(rows), "--dump-outputs", str(tmp_path / "out")]
    env = dict(os.environ)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "VROD_BENCH_FORCE_COLLECTIVE"):
        env.pop(v, None)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().split("\n") if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["ms_per_step"] > 0 and out["value"] > 0
    assert not {"cpu_baseline", "host_pointer_qps", "extra_hbm_1query", "recall_at_10"} & set(out)
    ids, sc = np.load(tmp_path / "out" / "ids.npy"), np.load(tmp_path / "out" / "scores.npy")
    assert ids.dtype == np.float64 and sc.dtype == np.float32 and ids.shape == sc.shape == (nq, k)
    va.load()
    dev = torch.device("cuda", 0)
    vi = torch.empty((nq, k), dtype=torch.int64, device=dev)
    vs = torch.empty((nq, k), dtype=torch.float32, device=dev)
    with va.Index(768, "bf16", "cosine", device=0) as ix:
        ix.add_synthetic(1, 0, rows)
        ix.search_synthetic_device(2, (warmup + steps - 1) * nq, nq, k, vi, vs)
    assert np.array_equal(ids, vi.cpu().numpy().astype(np.float64))
    assert np.array_equal(sc.view(np.uint32), vs.cpu().numpy().view(np.uint32))
