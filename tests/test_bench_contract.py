"""bench.py contract: one JSON line from rank 0 with the driver's fields, under
``torch.distributed.run`` with several ranks (gloo on the CPU; two ranks
sharing the one GPU over gloo on a GPU box — the 8-GPU RCCL run is the
driver's).  Rows are scaled down; the code path is the timed one."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(nproc, extra, env_extra=None, timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="2", **(env_extra or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", str(nproc), "--steps", "2", "--warmup", "1", "--full"] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert KEYS <= set(out)
    assert out["n_gpus"] == nproc and out["steps"] == 2 and out["warmup"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["config"]["parallelism"].startswith(f"dp{nproc}")
    return out


@pytest.mark.parametrize("model,extra", [
    ("gbm-higgs", ["--rows", "6000"]),
    ("dl-mlp", ["--rows", "2048", "--batch", "256"]),
])
def test_bench_two_ranks_cpu(model, extra):
    out = _run(2, ["--device", "cpu", "--model", model] + extra)
    if model == "gbm-higgs":
        assert out["scaling"] == "strong"          # headline default: 11M rows in total at every N
        assert out["config"]["global_batch"] == 6000 and out["config"]["rows_per_gpu"] == 3000
        assert 0.6 < out["train_auc"] <= 1.0
    else:
        assert out["config"]["global_batch"] == 512


def test_bench_plain_run_is_lean_and_dumps_its_outputs_cpu(tmp_path):
    """Without ``--full`` the run reports the timed steps only (no AUC, no
    instrumented steps, no end-to-end fit); ``--dump-outputs`` writes the
    margins and trees of the timed path, identical from run to run."""
    import numpy as np

    outs = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
               "--device", "cpu", "--rows", "6000", "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, OMP_NUM_THREADS="2"), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        outs.append(json.loads(lines[0]))
    out = outs[0]
    assert KEYS <= set(out)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(6000 / (out["ms_per_step"] / 1000.0))
    assert out["train_auc"] is None
    assert not {"fit_rows_per_s", "phase_us_per_tree", "host_enqueue_us_per_tree"} & set(out)
    assert sorted(os.listdir(tmp_path / "a")) == ["margin.npy", "trees.npy"]
    for name in ("margin.npy", "trees.npy"):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a, b)
    margin, trees = np.load(tmp_path / "a" / "margin.npy"), np.load(tmp_path / "a" / "trees.npy")
    assert margin.shape == (6000,) and np.isfinite(margin).all() and margin.std() > 0
    assert trees.shape[0] == 4 and trees.shape[2] == 6      # warm-up + timed trees
    assert (trees[:, 0, 0] >= 0).all()                      # every root splits


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_hip_engines_outputs(tmp_path):
    """HIP engine, plain run (graph replay, 4-tree groups): the dumped tree
    table holds the reachable nodes of the trees ``--dump-trees`` saves and
    zeros elsewhere, and there is one finite margin per training row."""
    import numpy as np

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "1",
           "--rows", "100003", "--dump-outputs", str(tmp_path / "out"), "--dump-trees", str(tmp_path / "trees.npy")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert KEYS <= set(out) and out["graph_replay"] and out["train_auc"] is None
    assert not {"fit_rows_per_s", "phase_us_per_tree"} & set(out)
    margin, table = np.load(tmp_path / "out" / "margin.npy"), np.load(tmp_path / "out" / "trees.npy")
    trees = np.load(tmp_path / "trees.npy")
    assert margin.dtype == np.float32 and margin.shape == (100003,) and np.isfinite(margin).all()
    assert table.dtype == np.float64 and table.shape == (7, trees.shape[1], 6)
    for t in range(7):
        keep = _reachable(trees[t])
        for j, f in enumerate(("feat", "bin", "na_left", "value")):
            np.testing.assert_array_equal(table[t, keep, j], trees[t][keep][f].astype(np.float64))
        rest = np.setdiff1d(np.arange(trees.shape[1]), keep)
        assert not table[t, rest].any()


@pytest.mark.gpu
def test_bench_two_ranks_one_gpu():
    """Two ranks on the one GPU (gloo carries the collectives): the weak-scaling
    GBM path of the driver's N>1 run, HIP kernels included."""
    out = _run(2, ["--model", "gbm-higgs", "--rows", "200000", "--scaling", "weak"], {"H2OMX_DIST_BACKEND": "gloo"},
               timeout=300)
    assert out["config"]["global_batch"] == 400000
    assert 0.6 < out["train_auc"] <= 1.0


def _reachable(tr):
    keep, stack = [], [0]
    while stack:
        i = stack.pop()
        keep.append(i)
        if tr[i]["feat"] >= 0:
            stack += [int(tr[i]["left"]), int(tr[i]["left"]) + 1]
    return sorted(keep)


def _assert_same_trees(a, b, exact_values):
    import numpy as np

    assert a.shape[0] == b.shape[0]
    for t in range(a.shape[0]):
        keep = _reachable(a[t])
        assert keep == _reachable(b[t]), f"tree {t} shape"
        for f in ("feat", "bin", "na_left"):
            np.testing.assert_array_equal(a[t][keep][f], b[t][keep][f], err_msg=f"tree {t} {f}")
        if exact_values:
            np.testing.assert_array_equal(a[t][keep]["value"], b[t][keep]["value"], err_msg=f"tree {t}")
        else:
            np.testing.assert_allclose(a[t][keep]["value"], b[t][keep]["value"], rtol=1e-5, atol=1e-7)


def test_bench_strong_two_ranks_reproduce_one_rank_cpu(tmp_path):
    """Strong scaling splits ONE data set over the ranks: the 2-rank run grows
    the 1-rank trees (CPU reference builder: identical splits, fp64 leaf sums
    equal to rounding since the all-reduce changes the summation order)."""
    import numpy as np

    extra = ["--device", "cpu", "--rows", "6000", "--scaling", "strong"]
    one, two = tmp_path / "one.npy", tmp_path / "two.npy"
    _run(1, extra + ["--dump-trees", str(one)])
    _run(2, extra + ["--dump-trees", str(two)])
    _assert_same_trees(np.load(one), np.load(two), exact_values=False)


@pytest.mark.gpu
def test_bench_strong_two_ranks_reproduce_one_rank_gpu(tmp_path):
    """HIP engine, two ranks sharing the GPU over gloo, strong scaling: the
    integer histograms and global-row-id dither make the 2-rank trees
    bit-identical to the 1-rank trees, with graph replay on (segments split
    at the collectives) as in the timed run."""
    import numpy as np

    extra = ["--rows", "300000", "--scaling", "strong", "--instrument-steps", "2", "--fit-trees", "0"]
    one, two = tmp_path / "one.npy", tmp_path / "two.npy"
    o1 = _run(1, extra + ["--dump-trees", str(one)], timeout=300)
    # P2P off: the segmented graph with host-issued gloo collectives (the RCCL
    # fallback's structure); tests/test_p2p_gpu.py covers the one-graph P2P path
    o2 = _run(2, extra + ["--dump-trees", str(two)], {"H2OMX_DIST_BACKEND": "gloo", "H2OMX_P2P": "0"}, timeout=300)
    assert o1["graph_replay"] and o2["graph_replay"]
    _assert_same_trees(np.load(one), np.load(two), exact_values=True)
    assert o1["train_auc"] == o2["train_auc"]
    for o in (o1, o2):
        for k in ("host_enqueue_us_per_tree", "small_kernel_us_per_tree", "allreduce_us_per_tree",
                  "phase_us_per_tree"):
            assert k in o, k
    assert o2["allreduce_calls_per_tree"] >= 6     # one per level + leaf sums
