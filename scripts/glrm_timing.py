"""GLRM with missing entries: the torch expressions against the ops.glrm kernels.

    python scripts/glrm_timing.py [--out profiles/r19/glrm.txt] [--small] [--arms a,b,...]

Protocol: medians of 7 after 2 warm-ups with min .. max, a fresh process per
arm, device events around the launches; host clock plus a synchronise for the
public fit.  Every arm prints the same process's Tensor.copy_ rate, the peak of
torch.cuda.max_memory_allocated over the step and the bytes of A it stands
against; kernel arms print the fp64 matrix rate, issued (padded tiles) and useful.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARMS = [f"{s}_{r}_k{k}" for s in ("x", "y") for k in (10, 32) for r in ("torch", "hip")] + [
    "big_hip_k10", "big_torch_k10", "fit_torch_k10", "fit_hip_k10"]
REPS, WARM = 7, 2
PEAK_TFLOPS = 78.6
LAM = 1e-8


def _events(fn, reps=REPS, warm=WARM):
    import torch

    ts = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(a.elapsed_time(b))
    return ts


def _host(fn):
    import torch

    ts = []
    for i in range(WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def _copy_rate(dev):
    import torch

    a = torch.empty(1 << 27, dtype=torch.float64, device=dev)
    b = torch.empty_like(a)
    ms = statistics.median(_events(lambda: b.copy_(a)))
    return 2 * a.numel() * 8 / ms / 1e9          # TB/s, read + write


def _data(n, p, k, dev, missing=0.2):
    """A [p][n] (zeros where missing), mask, X [k][n], Y [k][p], filled a column at a time."""
    import torch

    g = torch.Generator(device=dev).manual_seed(0)
    A = torch.empty((p, n), dtype=torch.float32, device=dev)
    mask = torch.empty((p, n), dtype=torch.bool, device=dev)
    for j in range(p):
        torch.ge(torch.rand(n, generator=g, device=dev), missing, out=mask[j])
        A[j] = torch.randn(n, generator=g, device=dev) * mask[j]
    X = torch.randn((k, n), generator=g, device=dev)
    Y = torch.randn((k, p), generator=g, device=dev)
    return A, mask, X, Y


def _rates(n, p, k, ms):
    tc = k * (k + 1) // 2 + k
    tiles = -(-(tc - k) // 16) + -(-k // 16)
    return {"useful_TFLOPs": 2 * n * p * tc / ms / 1e9, "issued_TFLOPs": 2 * n * p * tiles * 16 / ms / 1e9,
            "peak_TFLOPs": PEAK_TFLOPS}


def run_arm(arm: str, small: bool) -> dict:
    import torch

    from h2omx.frame.frame import Frame, Vec
    from h2omx.models import glrm as M
    from h2omx.models.glrm import H2OGeneralizedLowRankEstimator
    from h2omx.ops import glrm

    dev = torch.device("cuda", 0)
    kind, route, k = arm.split("_")
    k = int(k[1:])
    res = {"arm": arm, "copy_TBps": _copy_rate(dev)}
    p = 50
    n = {"x": 1_000_000, "y": 1_000_000, "fit": 1_000_000, "big": 400_000_000}[kind] // (100 if small else 1)
    A, mask, X, Y = _data(n, p, k, dev)
    res.update(shape=[n, p, k], A_bytes=4 * n * p, inputs_bytes=torch.cuda.memory_allocated(dev))
    if kind == "fit":
        if route == "torch":
            M.als_engine = lambda A, k: "torch"
        fr = Frame([Vec(f"c{j}", torch.where(mask[j], A[j], torch.nan), "real") for j in range(p)])
        del A, mask, X
        box = {}

        def fit():
            box["m"] = H2OGeneralizedLowRankEstimator(k=k, init="SVD", max_iterations=10, min_step_size=0).train(
                training_frame=fr)
        ts = _host(fit)
        res.update(als_engine=box["m"].timings["als_engine"], objective=box["m"].objective)
    else:
        if kind == "x":
            step = (lambda: glrm.masked_x(A, mask, Y, LAM)) if route == "hip" else (
                lambda: M._solve_x_torch(A, mask, Y, LAM))
        elif route == "hip":
            def step():
                return glrm.masked_y_terms(A, mask, X)
            res.update(slab_rows=glrm.y_slab_rows(n, p, k, torch.cuda.get_device_properties(dev).multi_processor_count),
                       part_share=f"1/{glrm.Y_PART_SHARE} of A_bytes")
        else:
            def step():
                return M._solve_y_terms_torch(A, mask, X)
        torch.cuda.reset_peak_memory_stats(dev)
        try:
            ts = _events(step, 1, 0) if kind == "big" else _events(step)
            if kind == "big" and route == "hip":    # the x-step of the same frame, timed once as well
                res.update(x_step_ms=_events(lambda: glrm.masked_x(A, mask, Y, LAM), 1, 0)[0])
        except torch.cuda.OutOfMemoryError as e:
            res.update(refused=str(e).splitlines()[0][:300])
            return res
        res.update(step_peak_bytes=torch.cuda.max_memory_allocated(dev) - res["inputs_bytes"])
        if route == "hip":
            res.update(_rates(n, p, k, statistics.median(ts)))
    res.update(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=ARMS)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "glrm.txt"))
    a = ap.parse_args(argv)
    if a.arm:
        print(json.dumps(run_arm(a.arm, a.small)))
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for arm in a.arms.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm] + (["--small"] if a.small else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(f"{arm}: exit {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
