"""GLRM with generalized losses: the tensor route against the ops.glrm loss kernels.

    python scripts/glrm_loss_timing.py [--out profiles/r23/glrm_loss.txt] [--small] [--arms a,b,...]

Protocol of scripts/glrm_timing.py (its helpers are used): medians of 7 after 2 warm-ups
with min .. max, a fresh process per arm, device events around each gradient call, host
clock plus a synchronise for the public fit; every arm prints the same process's
Tensor.copy_ rate and the peak of torch.cuda.max_memory_allocated over the step.  The
seven losses are cycled over the columns.  Shapes: 1M x 20 and 10M x 100, k = 5.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

from glrm_timing import ROOT, _copy_rate, _data, _events, _host

SHAPES = {"std": (1_000_000, 20, 5), "big": (10_000_000, 100, 5)}
ARMS = [f"{g}_{r}_{s}" for s in SHAPES for g in ("gx", "gy") for r in ("torch", "hip")] + ["fit_torch_std", "fit_hip_std"]


def run_arm(arm: str, small: bool) -> dict:
    import numpy as np
    import torch

    from h2omx.frame.frame import Frame, Vec
    from h2omx.models import glrm as M
    from h2omx.models.glrm import H2OGeneralizedLowRankEstimator
    from h2omx.ops import glrm

    dev = torch.device("cuda", 0)
    kind, route, shape = arm.split("_")
    n, p, k = SHAPES[shape]
    n //= 100 if small else 1
    res = {"arm": arm, "copy_TBps": _copy_rate(dev)}
    A, mask, X, Y = _data(n, p, k, dev)
    X /= k ** 0.5
    res.update(shape=[n, p, k], A_bytes=4 * n * p, inputs_bytes=torch.cuda.memory_allocated(dev))
    if kind == "fit":
        if route == "torch":
            M.loss_engine = lambda A, k: "proxgrad-torch"
        fr = Frame([Vec(f"c{j}", torch.where(mask[j], A[j], torch.nan), "real") for j in range(p)])
        del A, mask, X
        box = {}

        def fit():
            box["m"] = H2OGeneralizedLowRankEstimator(k=k, init="SVD", loss="Absolute", max_iterations=10,
                                                      min_step_size=0).train(training_frame=fr)
        torch.cuda.reset_peak_memory_stats(dev)
        ts = _host(fit)
        res.update(als_engine=box["m"].timings["als_engine"], objective=box["m"].objective,
                   updates=box["m"].timings["updates"],
                   fit_peak_bytes=torch.cuda.max_memory_allocated(dev) - res["inputs_bytes"])
    else:
        codes = np.arange(p, dtype=np.int32) % len(glrm.LOSSES)
        pars = np.where(codes == glrm.LOSSES["Periodic"], 2 * np.pi / 3, 0.0)
        cols = glrm.loss_columns(codes, pars, dev)
        wrt = kind[1]
        if route == "hip":
            def step():
                return (glrm.loss_grad_x if wrt == "x" else glrm.loss_grad_y)(A, mask, X, Y, *cols)
        else:
            def step():
                return M._loss_grad_torch(A, mask, X, Y, codes, pars, wrt)
        torch.cuda.reset_peak_memory_stats(dev)
        try:
            ts = _events(step)
        except torch.cuda.OutOfMemoryError as e:
            res.update(refused=str(e).splitlines()[0][:300])
            return res
        res.update(step_peak_bytes=torch.cuda.max_memory_allocated(dev) - res["inputs_bytes"])
    res.update(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=ARMS)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "glrm_loss.txt"))
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
