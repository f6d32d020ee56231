"""Leaf assignment, staged probabilities and feature frequencies: the per-tree tensor
bodies of h2omx.explain_more against the ops.walk kernel route.

    python scripts/walk_timing.py [--out profiles/r24/walk.txt] [--small] [--arms a,b,...]

Protocol: medians of 7 after 2 warm-ups with min .. max, a fresh process per arm,
device events around the calls, next to the same process's Tensor.copy_ rate.
Arms ``<rows>x<cols>d<depth>_<leaf|path|staged|freq>_<torch|hip>`` time the body of one
public method (``leaf``: Node_ID, ``path``: Path) on a binomial stand-in model of 50
complete trees with random splits; the packed ensemble of the ``hip`` route is built
once, before the timed calls, as it is cached on the ensemble.  Arms
``<rows>x<cols>d<depth>_ids_hip`` time ops.walk.leaf_ids alone.  (The ``_ids_stage`` and
``_ids_nostage`` lines of profiles/r24/walk.txt come from the build that still had the
double-buffered LDS stage for tree records; it lost both and was taken out.)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ["1000000x20d5", "100000x100d10"]
ARMS = [f"{s}_{m}_{r}" for s in SHAPES for m in ("leaf", "path", "staged", "freq") for r in ("torch", "hip")] + \
       [f"{s}_ids_hip" for s in ("1000000x20d5", "1000000x20d9")]
REPS, WARM, NTREES = 7, 2, 50


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


def _model(F: int, depth: int):
    """A binomial stand-in with 50 complete heap-ordered trees of random splits."""
    import numpy as np
    import torch

    from h2omx.models.base import ModelCategory
    from h2omx.models.tree.boost import TreeEnsemble
    from h2omx.models.tree.structs import TREE_NODE_DTYPE

    rng = np.random.default_rng(0)
    m, cap = (1 << depth) - 1, (2 << depth) - 1
    trees = np.zeros((NTREES, cap), TREE_NODE_DTYPE)
    trees["feat"] = -1
    trees["feat"][:, :m] = rng.integers(0, F, (NTREES, m))
    trees["thr"][:, :m] = rng.normal(size=(NTREES, m)) * 0.5
    trees["left"][:, :m] = 2 * np.arange(m) + 1
    trees["na_left"][:, :m] = rng.integers(0, 2, (NTREES, m))
    trees["value"] = rng.normal(size=(NTREES, cap)) * 0.1
    ens = TreeEnsemble(trees=trees, K=1, dist="bernoulli", init_f=np.zeros(1))

    def link(margin):
        p = torch.sigmoid(margin[0])
        return torch.stack([1 - p, p])

    return types.SimpleNamespace(ens=ens, x=[f"x{j}" for j in range(F)], _link=link, category=ModelCategory.BINOMIAL,
                                 algo="gbm")


def run_arm(arm: str, small: bool) -> dict:
    import torch

    from h2omx import explain_more as em
    from h2omx.ops import walk

    dev = torch.device("cuda", 0)
    res = {"arm": arm, "copy_TBps": _copy_rate(dev)}
    shape, method, route = arm.split("_")
    n, rest = shape.split("x")
    n, (F, depth) = int(n), map(int, rest.split("d"))
    if small:
        n //= 10
    model = _model(F, depth)
    X = torch.randn((F, n), generator=torch.Generator(device=dev).manual_seed(0), device=dev)
    X[:, ::17] = float("nan")
    if route == "torch":
        fn = {"leaf": lambda: em._leaf_torch(model, X, "Node_ID"), "path": lambda: em._leaf_torch(model, X, "Path"),
              "staged": lambda: em._staged_torch(model, X), "freq": lambda: em._frequencies_torch(model, X)}[method]
    else:
        plan = walk.pack_walk(model.ens, dev)
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        res.update(engine=em.walk_engine(model, X, path=method == "path"),
                   slab_trees=walk.walk_slab_trees(n, plan.T, cus), used=int(plan.used.max()))
        fn = {"leaf": lambda: em._leaf_hip(model, X, "Node_ID"), "path": lambda: em._leaf_hip(model, X, "Path"),
              "staged": lambda: em._staged_hip(model, X), "freq": lambda: em._frequencies_hip(model, X),
              "ids": lambda: walk.leaf_ids(X, plan)}[method]
    torch.cuda.synchronize()
    ts = _events(fn)
    res.update(shape=[n, F, depth], median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=ARMS)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "walk.txt"))
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
