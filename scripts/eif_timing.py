"""Extended Isolation Forest scoring: the GEMM-and-gather route against the ops.anomaly
walk kernels, and the sparse walk against the dense one.

    python scripts/eif_timing.py [--out profiles/r21/eif_score.txt] [--small] [--arms a,b,...]

Protocol: medians of 7 after 2 warm-ups with min .. max, a fresh process per arm,
device events around the launches, next to the same process's Tensor.copy_ rate.
Arms ``<rows>x<cols>e<extension_level>_<torch|hip>`` time
ExtendedIsolationForestModel._mean_length_torch against ops.anomaly.eif_mean_length on
the same frame (100 trees, sample_size 256, trained on the first 65536 rows), with the
peak device memory over the inputs (frame; for ``hip`` also the packed forest, which is
built once per model).  Arms ``sweepK<K>_<sparse|dense>`` run both walks on one
1M x 32 forest with K non-zeros per normal (extension_level K - 1); they set
EIF_SPARSE_MAX_K.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(1_000_000, 20, 0), (1_000_000, 20, 2), (1_000_000, 20, 19), (100_000, 100, 0), (100_000, 100, 99)]
ARMS = [f"{n}x{p}e{e}_{r}" for n, p, e in SHAPES for r in ("torch", "hip")] + \
       [f"sweepK{k}_{r}" for k in (4, 8, 16, 32) for r in ("sparse", "dense")]
REPS, WARM = 7, 2
TRAIN_ROWS = 65536


def _events(fn):
    import torch

    ts = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append(a.elapsed_time(b))
    return ts


def _copy_rate(dev):
    import torch

    a = torch.empty(1 << 27, dtype=torch.float64, device=dev)
    b = torch.empty_like(a)
    ms = statistics.median(_events(lambda: b.copy_(a)))
    return 2 * a.numel() * 8 / ms / 1e9          # TB/s, read + write


def run_arm(arm: str, small: bool) -> dict:
    import torch

    from h2omx.frame.frame import Frame, Vec
    from h2omx.models import H2OExtendedIsolationForestEstimator
    from h2omx.ops import anomaly

    dev = torch.device("cuda", 0)
    res = {"arm": arm, "copy_TBps": _copy_rate(dev)}
    shape, route = arm.split("_")
    if shape.startswith("sweepK"):
        n, p, ext = 1_000_000, 32, int(shape[6:]) - 1
        anomaly.EIF_SPARSE_MAX_K = 0 if route == "dense" else p
    else:
        n, rest = shape.split("x")
        n, (p, ext) = int(n), map(int, rest.split("e"))
    if small:
        n //= 10
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn((p, n), generator=g, device=dev)
    fr = Frame([Vec(f"x{j}", X[j], "real") for j in range(p)])
    head = Frame([Vec(f"x{j}", X[j, :TRAIN_ROWS].contiguous(), "real") for j in range(p)])
    m = H2OExtendedIsolationForestEstimator(ntrees=100, sample_size=256, extension_level=ext, seed=1).train(
        training_frame=head)
    del head
    if route == "torch":
        fn = lambda: m._mean_length_torch(fr)
    else:
        plan = m._plan(dev)
        Xraw = m.design.raw_matrix(fr)
        fn = lambda: anomaly.eif_mean_length(Xraw, plan)
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        res.update(K=plan.K, dense=anomaly.eif_dense(plan), slab_trees=anomaly.eif_slab_trees(
            n, 100, p, cus, anomaly.EIF_DENSE_ROWS if anomaly.eif_dense(plan) else anomaly.EIF_SPARSE_ROWS))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ts = _events(fn)
    res.update(shape=[n, p, ext], limit=m.limit, peak_bytes_over_inputs=torch.cuda.max_memory_allocated(dev) - base,
               median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=ARMS)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "eif_score.txt"))
    a = ap.parse_args(argv)
    if a.arm:
        print(json.dumps(run_arm(a.arm, a.small)))
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for arm in a.arms.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm] + (["--small"] if a.small else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:       # a failed arm ends the run: nothing more is started on the device
                print(f"{arm}: exit {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
