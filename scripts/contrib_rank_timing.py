"""Time the ranked-contribution kernel against the same ranking through
``torch.sort`` and against the SHAP kernel whose output it ranks.

Two shapes: the contribution planes of a GBM (50 trees, depth 5, 28 features,
seeded synthetic data) on 100k rows, and a synthetic [100][1M] plane of normal
floats.  Two requests: ``top_n=3, bottom_n=3`` and ``top_n=-1`` (all features,
descending).  One arm per process:

  shap    h2omx_tree_shap alone, for scale (GBM shape only)
  sort    torch.sort(stable=True) of the keys along the feature axis, descending
          and (for bottom_n) ascending, the slices and the cast that give the
          same [kt + kb][n] index and value planes; checked equal to the kernel's
  rank    h2omx_contrib_rank, output buffers allocated once
  public  model.predict_contributions(frame, top_n=..) wall time ending in a
          synchronise, next to the unsorted call (GBM shape only)

Per arm: warm-up calls, then repeated calls with device events around the
launches (``public``: a host clock).  Reported: median and min .. max.

    python scripts/contrib_rank_timing.py --out profiles/r12/contrib_rank.txt
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

RUNS = (("shap", "gbm"), ("sort", "gbm"), ("rank", "gbm"), ("public", "gbm"), ("sort", "synthetic"),
        ("rank", "synthetic"))
REQUESTS = {"top3_bottom3": (3, 3), "all_descending": (-1, None)}


def _sort_rank(phi, kt: int, kb: int):
    """The ranking of ``_rank_numpy`` through torch: stable sorts keep ties in
    index order in both directions."""
    import torch

    idx, val = [], []
    if kt:
        v, i = torch.sort(phi, dim=0, descending=True, stable=True)
        idx.append(i[:kt])
        val.append(v[:kt])
    if kb:
        v, i = torch.sort(phi, dim=0, descending=False, stable=True)
        idx.append(i[:kb])
        val.append(v[:kb])
    return torch.cat(idx).to(torch.int32), torch.cat(val)


def _arm(arm: str, shape: str, rows: int, warmup: int, repeats: int) -> dict:
    import numpy as np
    import torch

    from h2omx import explain as ex
    from h2omx.frame import Frame
    from h2omx.models import H2OGradientBoostingEstimator
    from h2omx.ops import P, check, explain_lib, stream

    dev = torch.device("cuda", 0)
    lib = explain_lib()
    info = {"arm": arm, "shape": shape}
    g = torch.Generator(device=dev).manual_seed(7)
    if shape == "gbm":
        F = 28
        X = torch.randn((rows, F), generator=g, device=dev)
        y = ((X[:, 0] + X[:, 1] * X[:, 2] - 0.5 * X[:, 3] + torch.randn(rows, generator=g, device=dev)) > 0).float()
        full = Frame.from_tensor(X.t().contiguous(), y=y, y_categorical=True)
        full.vecs[-1].domain = ["0", "1"]
        names = full.names[:-1]
        m = H2OGradientBoostingEstimator(ntrees=50, max_depth=5, seed=1).train(y=full.names[-1], training_frame=full)
        xs = Frame([v for v in full.vecs if v.name in names])
        plain = ex.predict_contributions(m, xs)
        phi = torch.stack([plain.vec(c).data for c in m.x]).contiguous()
    else:
        F = 100
        phi = torch.randn((F, 10 * rows), generator=g, device=dev)
    n = int(phi.shape[1])
    info.update(F=F, rows=n)

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
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

    if arm == "shap":
        nt = m.ens.ntrees
        lv, el, _, maxm, sets = ex.tree_paths(m.ens.trees[:nt], 1.0)
        fr = m.adapt_frame(xs)
        Xc = (m._matrix(fr) if hasattr(m, "_matrix") else fr.feature_matrix(m.x)).float().contiguous()
        L = int(lv.shape[0])
        lvd = torch.from_numpy(lv).to(dev)
        eld = torch.from_numpy(el).to(dev)
        setd = torch.from_numpy(sets.view(np.int32).copy()).to(dev)
        wt = torch.from_numpy(ex.shapley_weights(ex._bucket(maxm)).astype(np.float32)).to(dev)
        out = torch.zeros((F, n), dtype=torch.float32, device=dev)
        info["leaves"] = L
        info["ms"] = {"tree_shap": series(events, lambda: check(lib.h2omx_tree_shap(
            P(Xc), Xc.stride(0), n, F, P(lvd), L, P(eld), P(wt), maxm, P(out), P(setd), stream(dev)), "tree_shap"))}
        return info
    if arm == "public":
        info["ms"] = {"unsorted": series(wall, lambda: m.predict_contributions(xs))}
        for name, (t, b) in REQUESTS.items():
            info["ms"][name] = series(wall, lambda: m.predict_contributions(xs, top_n=t, bottom_n=b))
        return info
    info["ms"] = {}
    for name, (t, b) in REQUESTS.items():
        kt, kb = ex._rank_spec(t, b, F)
        want_idx, want_val = ex._rank_device(phi, kt, kb, False)
        if arm == "sort":
            idx, val = _sort_rank(phi, kt, kb)
            if not (torch.equal(idx, want_idx) and torch.equal(val, want_val)):
                raise SystemExit(f"{shape} {name}: the torch.sort ranking differs from the kernel's")
            del idx, val
            info["ms"][name] = series(events, lambda: _sort_rank(phi, kt, kb))
        else:
            idx, val = torch.empty_like(want_idx), torch.empty_like(want_val)
            info["ms"][name] = series(events, lambda: check(lib.h2omx_contrib_rank(
                P(phi), n, n, F, kt, kb, 0, P(idx), P(val), stream(dev)), "contrib_rank"))
            if not (torch.equal(idx, want_idx) and torch.equal(val, want_val)):
                raise SystemExit(f"{shape} {name}: two kernel calls differ")
    return info


def _fmt(v):
    return f"{statistics.median(v):10.3f}  [{min(v):.3f} .. {max(v):.3f}]"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100_000, help="GBM rows; the synthetic plane has ten times as many")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "contrib_rank.txt"))
    ap.add_argument("--arm", choices=sorted({r[0] for r in RUNS}), help="run one arm in this process")
    ap.add_argument("--shape", choices=("gbm", "synthetic"), default="gbm")
    a = ap.parse_args()
    if a.arm:
        print("RESULT " + json.dumps(_arm(a.arm, a.shape, a.rows, a.warmup, a.repeats)), flush=True)
        return
    res = {}
    for arm, shape in RUNS:                       # a fresh process per arm, each under its own time limit
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--shape", shape,
                            "--rows", str(a.rows), "--warmup", str(a.warmup), "--repeats", str(a.repeats)],
                           stdout=subprocess.PIPE, text=True, timeout=300)
        if p.returncode != 0:
            raise SystemExit(f"arm {arm} ({shape}) failed with status {p.returncode}")
        res[arm, shape] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    lines = ["# ranked contributions: h2omx_contrib_rank against torch.sort(stable=True) and the SHAP kernel",
             f"# {a.warmup} warm-up + {a.repeats} timed calls per arm, a fresh process per arm; ms, median [min .. max]",
             "# shap / sort / rank: device events around the launches; public: host clock + synchronise"]
    for shape in ("gbm", "synthetic"):
        r0 = res["rank", shape]
        what = "GBM 50 trees depth 5" if shape == "gbm" else "normal floats"
        lines.append(f"## {shape}: {what}, [{r0['F']}][{r0['rows']}] planes")
        for arm, sh in RUNS:
            if sh != shape:
                continue
            for name, v in res[arm, sh]["ms"].items():
                lines.append(f"{arm:7s} {name:15s} {_fmt(v):>40s}")
        for name in REQUESTS:
            s, k = res["sort", shape]["ms"][name], res["rank", shape]["ms"][name]
            sm, km = statistics.median(s), statistics.median(k)
            spread = max(max(s) - min(s), max(k) - min(k))
            lines.append(f"{name}: kernel {km:.3f} ms, torch.sort {sm:.3f} ms ({sm / km:.1f} x); the difference is "
                         f"{'more' if sm - km > spread else 'NOT more'} than both arms' min .. max spreads "
                         f"({spread:.3f} ms)")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt)
    print(txt, end="")


if __name__ == "__main__":
    main()
