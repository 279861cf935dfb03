"""bench.py prints ONE JSON line with the fields the driver and the judge read."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_has_the_contract_fields():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--no-euclid"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    b = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in b, key
    assert b["n_gpus"] == 1 and b["steps"] == 2 and b["warmup"] == 1 and b["higher_is_better"] is True
    assert b["value"] > 0 and abs(b["value"] - 1e3 / b["ms_per_step"]) / b["value"] < 1e-6
    assert "workload" in b["config"] and "model" not in b["config"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in b["roofline"], key
    assert abs(b["roofline"]["frac"] - b["roofline"]["achieved"] / b["roofline"]["peak"]) < 1e-9
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in b["cpu_baseline"], key
    assert b["cpu_baseline"]["kind"] in ("port", "reference")
    assert b["errors_vs_bruteforce"] <= 504   # no worse than the reference's own run


@pytest.mark.gpu
def test_bench_two_ranks_sharing_the_gpu_headlines_the_row_sharded_build():
    """--gpus 2 rehearsal on the one GPU of the test box (gloo, both ranks on GPU 0): the headline is the
    row-sharded Euclidean build (strong scaling), with recall and the single-GPU time of the same workload."""
    import socket

    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--steps", "2",
                        "--warmup", "1", "--share-gpu", "--euclid-rows", "200000"], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, lines
    b = json.loads(lines[0])
    assert b["n_gpus"] == 2 and b["scaling"] == "strong" and b["config"]["total_rows"] == 200000
    assert "rows sharded" in b["config"]["parallelism"]
    assert b["value"] > 0 and abs(b["value"] - 1e3 / b["ms_per_step"]) / b["value"] < 1e-6
    assert b["recall_at_k"] >= 0.9
    assert b["single_gpu_same_workload"]["fit_time_s"] > 0
    assert abs(b["value_single_gpu_same_workload"] - 1.0 / b["single_gpu_same_workload"]["fit_time_s"]) < 1e-9
    assert "NOT the --gpus 1 default workload" in b["config"]["workload"]
    assert b["strings_replicas"]["errors_vs_bruteforce"] <= 504


@pytest.mark.gpu
def test_bench_plain_shell_gpus_2_launches_its_own_ranks():
    """`python bench.py --gpus 2 --share-gpu --backend gloo` from a plain shell (no launcher, no WORLD_SIZE): the process
    starts its two ranks itself and passes their one JSON line through."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--share-gpu", "--backend", "gloo", "--steps", "1",
                        "--warmup", "1", "--euclid-rows", "100000"], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, lines
    b = json.loads(lines[0])
    assert b["n_gpus"] == 2 and b["scaling"] == "strong" and b["value"] > 0 and b["value_single_gpu_same_workload"] > 0


def test_bench_self_launch_command_line():
    """CPU: the launcher branch builds the driver's command line (torch.distributed.run, one process per GPU, 127.0.0.1) and is
    taken only without WORLD_SIZE."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'args.gpus > 1 and "WORLD_SIZE" not in os.environ' in src
    assert '"--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1"' in src
    assert "assert args.gpus == world" in src   # (a launcher that was given another world size is still refused)


# keys only `--full` measures (CPU baselines, kernel events / roofline, recall, the other workloads)
FULL_ONLY = ("cpu_baseline", "cpu_baseline_python_metric", "roofline", "kernels", "errors_vs_bruteforce", "recall_at_k",
             "c2_device_sampler_plugin", "c4_digits_wasserstein", "pairlist_kernels_at_scale", "levenshtein_100k_thinned_pairlist",
             "c3_euclid_streamed")


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_and_dumps_the_last_graph(tmp_path):
    """A plain run prints the headline only, times exactly --steps fits, and --dump-outputs writes the last timed fit's graph
    (float64 .npy, well under 64 MB); two runs with the same arguments write the same graph, and it is the headline
    workload's: no worse against brute force than the reference's own run."""
    from annchor_amd import compare_neighbor_graphs

    graphs = []
    for i in range(2):
        d = tmp_path / ("out%d" % i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(d)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        b = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in b, key
        assert b["steps"] == 3 and b["warmup"] == 1 and b["unit"] == "graphs/s" and b["higher_is_better"] is True
        assert b["value"] > 0 and abs(b["value"] - 1e3 / b["ms_per_step"]) / b["value"] < 1e-6
        for key in FULL_ONLY:
            assert key not in b, key
        names = sorted(f.name for f in d.iterdir())
        assert names == ["neighbor_graph_distances.npy", "neighbor_graph_indices.npy"], names
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
        idx, dist = np.load(d / "neighbor_graph_indices.npy"), np.load(d / "neighbor_graph_distances.npy")
        assert idx.dtype == np.float64 and dist.dtype == np.float64 and idx.shape == dist.shape == (1600, 25)
        assert np.array_equal(idx, np.round(idx)) and idx.min() >= 0 and idx.max() < 1600
        graphs.append((idx, dist))
    assert np.array_equal(graphs[0][0], graphs[1][0]) and np.array_equal(graphs[0][1], graphs[1][1])
    G = np.load(os.path.join(ROOT, "tests", "golden", "strings_full.npz"))
    truth = (G["truth_idx"].astype(np.int64), G["truth_dist"].astype(np.float64))
    assert compare_neighbor_graphs(truth, (graphs[0][0].astype(np.int64), graphs[0][1]), 25) <= 504


def test_bench_options():
    """CPU: --full and --dump-outputs exist (parsed before any GPU work: --help needs none)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
