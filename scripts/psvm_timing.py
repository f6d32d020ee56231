"""PSVM timings: the torch route against the ops.svm kernels.

    python scripts/psvm_timing.py [--out profiles/r18/psvm.txt] [--small]
    python scripts/psvm_timing.py --out profiles/r20/psvm_score.txt --arms \
        score_torch,score_hip,score1m_torch,score1m_hip,scorefew_torch,scorefew_hip,fit1m_hip

Protocol: medians of 7 after 2 warm-ups with min .. max, a fresh process per
arm, device events around the launches; host clock plus a synchronise for the
public fit.  Bandwidths stand next to the same process's Tensor.copy_ rate.
The scoring arms time PSVMModel._decision_torch against ops.svm.rbf_decision on
the same tensors: ``score`` on the support vectors of the 100k x 20 fit,
``score1m`` on 1M x 20 synthetic rows against 50k synthetic support vectors,
``scorefew`` on 100k x 20 rows against 64.
``fit1m`` is the public fit at 1M x 20 (medians of 3 after 1 warm-up: a fit
takes seconds).  An allocator refusal is recorded, not raised.
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

ARMS = ["icf_torch", "icf_hip", "gram_torch", "gram_hip", "iter_torch", "iter_hip", "fit_torch", "fit_hip"]
SCORE_ARMS = ["score_torch", "score_hip", "score1m_torch", "score1m_hip", "scorefew_torch", "scorefew_hip", "fit1m_hip"]
REPS, WARM = 7, 2


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


def _host(fn, reps=REPS, warm=WARM):
    import torch

    ts = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def _copy_rate(dev):
    import torch

    a = torch.empty(1 << 27, dtype=torch.float64, device=dev)
    b = torch.empty_like(a)
    ms = statistics.median(_events(lambda: b.copy_(a)))
    return 2 * a.numel() * 8 / ms / 1e9          # TB/s, read + write


def _blobs(n, d, dev, seed=0):
    import torch

    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn((n, d), generator=g, dtype=torch.float64, device=dev)
    y = torch.where((X[:, :2] ** 2).sum(1) < 1.4, 1.0, -1.0).double()
    return X, y


def _score_arm(kind: str, route: str, small: bool, dev, res: dict):
    """Decision values without b on device tensors; returns the event timings."""
    import torch

    from h2omx.frame.frame import ENUM, Frame, Vec
    from h2omx.models import H2OSupportVectorMachineEstimator
    from h2omx.models import psvm
    from h2omx.ops import svm

    d = 20
    if kind == "score":
        n = 50_000 if small else 100_000
        Xd, y = _blobs(n, d, dev)
        fr = Frame([Vec(f"x{j}", Xd[:, j].float().contiguous(), "real") for j in range(d)]
                   + [Vec("y", (y > 0).int(), ENUM, ["0", "1"])])
        m = H2OSupportVectorMachineEstimator(max_iterations=50).train(y="y", training_frame=fr)
        X = psvm._design(fr, m.x, m.means, m.scales).float()
        del Xd, fr
    else:
        n, nsv = (100_000, 64) if kind == "scorefew" else (100_000, 5_000) if small else (1_000_000, 50_000)
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn((n, d), generator=g, device=dev)
        m = psvm.PSVMModel.__new__(psvm.PSVMModel)
        m.sv = torch.randn((nsv, d), generator=g, device=dev)
        m.coef = torch.randn(nsv, generator=g, dtype=torch.float64, device=dev)
        m.gamma = 1.0 / d
    S, coef = m.sv.to(dev), m.coef.to(dev)
    nsv = S.shape[0]
    fn = (lambda: m._decision_torch(X)) if route == "torch" else (lambda: svm.rbf_decision(X, S, coef, m.gamma))
    tiles = -(-n // 64) * -(-nsv // 64)
    res.update(shape=[n, nsv, d], pairs=n * nsv, issued_flop=2 * 64 * 64 * 4 * -(-d // 4) * tiles,
               variant_libs=bool(os.environ.get("H2OMX_LIB_DIR")))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    try:
        ts = _events(fn)
    except torch.OutOfMemoryError as e:
        res.update(error=str(e)[:400])
        return None
    res.update(peak_bytes_over_inputs=torch.cuda.max_memory_allocated(dev) - base)
    return ts


def run_arm(arm: str, small: bool) -> dict:
    import torch

    from h2omx.frame.frame import ENUM, Frame, Vec
    from h2omx.models import H2OSupportVectorMachineEstimator
    from h2omx.models import psvm
    from h2omx.ops import svm

    dev = torch.device("cuda", 0)
    kind, route = arm.split("_")
    res = {"arm": arm, "copy_TBps": _copy_rate(dev)}
    if route == "torch":        # the route of a CPU frame, on device tensors
        psvm.icf_engine = lambda X, p, comm=None: "torch"
        psvm.ipm_engine = lambda H: "torch"
    if kind in ("score", "score1m", "scorefew"):
        ts = _score_arm(kind, route, small, dev, res)
        if ts is None:
            return res
    elif kind == "icf":
        n, d, p = (20_000, 20, 142) if small else (200_000, 20, 448)
        X, _ = _blobs(n, d, dev)
        ts = _events(lambda: psvm.icf(X, 1.0 / d, p, 1e-5))
        k = psvm.icf(X, 1.0 / d, p, 1e-5).shape[1]
        res.update(shape=[n, d, p], k_used=k, doubles_read=n * k * k / 2 + n * k * d)
    elif kind == "gram":
        n, k = (100_000, 300) if small else (1_000_000, 1000)
        H, y = _blobs(n, k, dev)
        Dg = torch.rand(n, dtype=torch.float64, device=dev) + 0.5
        if route == "torch":
            def gram():
                Hy = H * y[:, None]
                Hd = Hy / Dg[:, None]
                return Hy.t() @ Hd
        else:
            def gram():
                return svm.wsyrk(H, 1.0 / Dg)
        ts = _events(gram)
        nb = -(-k // 64)
        res.update(shape=[n, k], useful_flop=n * k * (k + 1), full_flop=2 * n * k * k,
                   issued_flop=2 * n * 64 * 64 * (nb * (nb + 1) // 2 - nb / 4))
    else:
        # the fit scores its training frame: on the torch route the [rows][nsv] fp64 blocks bound the shape
        n, d = (50_000, 20) if small else (100_000, 20) if kind == "fit" else (1_000_000, 20)
        X, y = _blobs(n, d, dev)
        fr = Frame([Vec(f"x{j}", X[:, j].float().contiguous(), "real") for j in range(d)]
                   + [Vec("y", (y > 0).int(), ENUM, ["0", "1"])])
        if kind in ("fit", "fit1m"):
            box = {}

            def fit():
                box["m"] = H2OSupportVectorMachineEstimator(max_iterations=50).train(y="y", training_frame=fr)
            ts = _host(fit) if kind == "fit" else _host(fit, 3, 1)
            res.update(shape=[n, d], timings=box["m"].timings, nsv=int(box["m"].sv.shape[0]))
        else:                   # one interior-point iteration on the factor of the same frame
            p = int(-(-n ** 0.5 // 1))
            H = psvm.icf(X, 1.0 / d, p, 1e-5)
            est = H2OSupportVectorMachineEstimator(max_iterations=1)
            C = torch.ones(n, dtype=torch.float64, device=dev)
            ts = _events(lambda: est._ipm(H, y, C, None))
            res.update(shape=list(H.shape))
    res.update(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=ARMS + SCORE_ARMS)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "psvm.txt"))
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
