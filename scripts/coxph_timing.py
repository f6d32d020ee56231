"""Time the CoxPH Newton pass and concordance (round 12's protocol: a fresh
process per arm, warm-ups, then repeats with device events around the launches;
the public fit: host clock ending in a synchronise; median and min .. max).

  parent_pass   models.coxph._event_sums, 200k x 20, Efron, 200 distinct times
  hip_pass      ops.survival.cox_newton_pass on the same data (checked against
                the parent arm's formulas by the test suite, not here)
  kernels       10M x 50, 1000 distinct times: row pass, X'WX on the fp64 matrix
                units, the whole pass, and Tensor.copy_ of X as the stream yardstick
  conc_torch    the torch pair tables, 200k rows
  conc_hip      h2omx_cox_concordance, 200k rows
  public        H2OCoxProportionalHazardsEstimator.train, 1M x 20

    python scripts/coxph_timing.py --out profiles/r17/coxph.txt
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
sys.path.insert(0, ROOT)

ARMS = ("parent_pass", "hip_pass", "kernels", "conc_torch", "conc_hip", "public")
FP64_MATRIX_PEAK = 78.6e12   # MI355X, FLOP/s (vendor figure)


def _data(n, p, distinct, dev, seed=5):
    import torch

    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn((n, p), generator=g, device=dev, dtype=torch.float64)
    t = -torch.log(torch.rand(n, generator=g, device=dev, dtype=torch.float64)) * torch.exp(-0.5 * X[:, 0])
    t = torch.ceil(t / t.max() * distinct * 20).clamp_max(distinct)
    d = (torch.rand(n, generator=g, device=dev) < 0.6).double()
    X = X - X.mean(0)
    beta = torch.randn(p, generator=g, device=dev, dtype=torch.float64)
    return X, t, d, torch.ones_like(t), torch.zeros(n, dtype=torch.long, device=dev), beta / beta.norm()


def _arm(arm: str, warmup: int, repeats: int) -> dict:
    import torch

    from h2omx.models import coxph
    from h2omx.ops import survival

    dev = torch.device("cuda", 0)
    info = {"arm": arm, "ms": {}}

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize(dev)
        del r
        return a.elapsed_time(b)

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize(dev)
        del r
        return (time.perf_counter() - t0) * 1e3

    def series(timer, fn):
        for _ in range(warmup):
            timer(fn)
        return [timer(fn) for _ in range(repeats)]

    if arm in ("parent_pass", "hip_pass"):
        X, t, d, w, s, beta = _data(200_000, 20, 200, dev)
        if arm == "parent_pass":
            fn = lambda: coxph._event_sums(t, None, d, w, X @ beta, X, s, True)   # noqa: E731
        else:
            plan = survival.cox_prepare(t, None, d, w, s, X)
            fn = lambda: survival.cox_newton_pass(plan, beta, True)               # noqa: E731
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        info["ms"]["pass 200k x 20"] = series(events, fn)
        info["peak_bytes"] = torch.cuda.max_memory_allocated(dev) - base
    elif arm == "kernels":
        n, p = 10_000_000, 50
        X, t, d, w, s, beta = _data(n, p, 1000, dev)
        plan = survival.cox_prepare(t, None, d, w, s, X)
        del X
        lib = survival.survival_lib()
        eta, r = torch.empty_like(plan.w), torch.empty_like(plan.w)
        info["ms"]["row pass + fold 10M x 50"] = series(
            events, lambda: survival._row_sums(lib, plan, None, plan.b, beta, eta, r, True))
        info["ms"]["wxty (X, X, omega) 10M x 50"] = series(events, lambda: survival.wxty(plan.Xs, plan.Xs, r))
        info["ms"]["whole pass 10M x 50"] = series(events, lambda: survival.cox_newton_pass(plan, beta, True))
        Y = torch.empty_like(plan.Xs)
        info["ms"]["copy_ of X (4 GB -> 4 GB)"] = series(events, lambda: Y.copy_(plan.Xs))
        info["nb"] = plan.nb
    elif arm in ("conc_torch", "conc_hip"):
        X, t, d, w, s, beta = _data(200_000, 20, 200, dev)
        lp = torch.round(X @ beta, decimals=2)
        fn = coxph._concordance_torch if arm == "conc_torch" else survival.concordance
        info["value"] = fn(t, d, lp)
        info["ms"]["concordance 200k"] = series(wall, lambda: fn(t, d, lp))
    else:
        import numpy as np
        import pandas as pd

        from h2omx.frame import Frame
        from h2omx.models import H2OCoxProportionalHazardsEstimator

        X, t, d, w, s, beta = _data(1_000_000, 20, 1000, dev)
        df = pd.DataFrame(X.cpu().numpy().astype(np.float32), columns=[f"x{j}" for j in range(20)])
        df["t"], df["ev"] = t.cpu().numpy(), d.cpu().numpy()
        fr = Frame.from_pandas(df, device="cuda")
        info["ms"]["fit 1M x 20"] = series(wall, lambda: H2OCoxProportionalHazardsEstimator(stop_column="t").train(
            x=[f"x{j}" for j in range(20)], y="ev", training_frame=fr))
    return info


def _fmt(v):
    return f"{statistics.median(v):10.3f}  [{min(v):.3f} .. {max(v):.3f}]"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "coxph.txt"))
    ap.add_argument("--arm", choices=ARMS, help="run one arm in this process")
    a = ap.parse_args()
    if a.arm:
        print("RESULT " + json.dumps(_arm(a.arm, a.warmup, a.repeats)), flush=True)
        return
    res = {}
    for arm in ARMS:                                  # a fresh process per arm, each under its own time limit
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--warmup", str(a.warmup),
                            "--repeats", str(a.repeats)], stdout=subprocess.PIPE, text=True, timeout=280)
        if p.returncode != 0:
            raise SystemExit(f"arm {arm} failed with status {p.returncode}")
        res[arm] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    lines = ["# CoxPH: Newton pass (Efron) and concordance",
             f"# {a.warmup} warm-up + {a.repeats} timed calls per arm, a fresh process per arm; ms, median [min .. max]"]
    for arm in ARMS:
        for name, v in res[arm]["ms"].items():
            lines.append(f"{arm:12s} {name:30s} {_fmt(v):>44s}")
    pm, hm = res["parent_pass"]["ms"]["pass 200k x 20"], res["hip_pass"]["ms"]["pass 200k x 20"]
    lines.append(f"peak device memory of a pass, 200k x 20: parent {res['parent_pass']['peak_bytes'] / 2**20:.0f} MiB, "
                 f"kernels {res['hip_pass']['peak_bytes'] / 2**20:.0f} MiB")
    if min(pm) > max(hm):
        lines.append(f"pass 200k x 20: the ranges do not overlap, parent / kernels = "
                     f"{statistics.median(pm) / statistics.median(hm):.1f} x")
    else:
        lines.append("pass 200k x 20: the ranges overlap, no ratio stated")
    k = res["kernels"]["ms"]
    n, p = 10_000_000, 50
    cp = statistics.median(k["copy_ of X (4 GB -> 4 GB)"])
    rp = statistics.median(k["row pass + fold 10M x 50"])
    wx = statistics.median(k["wxty (X, X, omega) 10M x 50"])
    T = -(-p // 16)
    issued = 2.0 * n * 256 * (T * (T + 1) // 2)       # FLOP the instruction issues, padded tiles, upper triangle
    lines.append(f"copy_ moves {2 * 8 * n * p / cp / 1e9:.2f} TB/s (read + write); the row pass reads X once: "
                 f"{8 * n * p / rp / 1e9:.2f} TB/s ({rp / (cp / 2) * 100:.0f} % of the time copy_ needs per 4 GB)")
    lines.append(f"wxty: {issued / wx / 1e9:.1f} TFLOP/s issued ({issued / wx / 1e9 / (FP64_MATRIX_PEAK / 1e12) * 100:.1f} % "
                 f"of the {FP64_MATRIX_PEAK / 1e12:.1f} TFLOP/s fp64 matrix peak), {n * p * (p + 1) / wx / 1e9:.1f} TFLOP/s "
                 f"useful; buckets {res['kernels']['nb']}")
    lines.append(f"concordance 200k: torch {res['conc_torch']['value']!r}, kernel {res['conc_hip']['value']!r}")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt)
    print(txt, end="")


if __name__ == "__main__":
    main()
