"""Time the partial dependence sweep kernel against one scoring launch per cell.

One GBM (50 trees, depth 5, 28 features, seeded synthetic data) and 100k rows;
the swept column is the most important feature (varimp), the pair adds the
second; 20 grid values per column.  One arm per process:

  a  20 launches of h2omx_predict_raw on matrices with the column overwritten
     (what a 1-D table cost before the sweep kernel)
  b  h2omx_pd_sweep for the same 20 cells
  c  400 launches of h2omx_predict_raw (both columns overwritten)
  d  h2omx_pd_sweep for the 20 x 20 table (20 slices of the pinned column)
  e  the public 1-D call as it stood before: the frame-substitution loop with
     one predict_raw and one moment reduction per cell (kept here verbatim)
  f  the public 1-D call, model.partial_dependence

a - d: device events around the launches alone (buffers allocated, node table
and grid uploaded once; the row fill and the margin initialisation are inside,
as both ways need them).  e, f: a host clock around the call ending in a
synchronise.  Per arm: warm-up calls, then repeated calls; reported are the
median and min .. max, and for b and d the mean number of root-to-leaf walks
per (row, tree) from the kernel's counting instantiation (a separate call).

    python scripts/partial_dependence_timing.py --out profiles/r11/partial_dependence.txt
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("a", "b", "c", "d", "e", "f")
NBINS = 20


def _loop_partial_dependence(model, frame, col, nbins=20, target=None):
    """The 1-D table as computed before the sweep kernel (arm e)."""
    import numpy as np
    import torch

    from h2omx.explain import _response
    from h2omx.frame.frame import Frame, Vec

    frame = model.adapt_frame(frame)
    v = frame.vec(col)
    n = frame.nrows
    x = v.as_float()
    ok = ~torch.isnan(x)
    lo_v, hi_v = float(x[ok].min().float()), float(x[ok].max().float())
    grid = list(np.linspace(lo_v, hi_v, nbins)) if hi_v > lo_v else [lo_v]
    rows = []
    for g in grid:
        nv = Vec(col, torch.full((n,), float(g), dtype=torch.float32, device=v.data.device), v.vtype)
        fr = Frame([nv if u.name == col else u for u in frame.vecs])
        r = _response(model, model.predict_raw(fr), target).double()
        st = torch.stack([r.sum(), (r * r).sum(), torch.tensor(float(n), dtype=torch.float64, device=r.device)])
        s, s2, cnt = (float(a) for a in st)
        mean = s / max(cnt, 1.0)
        sd = math.sqrt(max(s2 / max(cnt, 1.0) - mean * mean, 0.0) * cnt / max(cnt - 1.0, 1.0))
        rows.append({col: g, "mean_response": mean, "stddev_response": sd,
                     "std_error_mean_response": sd / math.sqrt(max(cnt, 1.0))})
    return {"column": col, "target": target, "data": rows}


def _arm(arm: str, rows: int, warmup: int, repeats: int) -> dict:
    import numpy as np
    import torch

    from h2omx import explain as ex
    from h2omx.frame import Frame
    from h2omx.models import H2OGradientBoostingEstimator
    from h2omx.ops import P, check, explain_lib, stream, tree_lib

    dev = torch.device("cuda", 0)
    F = 28
    g = torch.Generator(device=dev).manual_seed(7)
    X = torch.randn((rows, F), generator=g, device=dev)
    y = ((X[:, 0] + X[:, 1] * X[:, 2] - 0.5 * X[:, 3] + torch.randn(rows, generator=g, device=dev)) > 0).float()
    full = Frame.from_tensor(X.t().contiguous(), y=y, y_categorical=True)
    full.vecs[-1].domain = ["0", "1"]
    names = full.names[:-1]
    m = H2OGradientBoostingEstimator(ntrees=50, max_depth=5, seed=1).train(y=full.names[-1], training_frame=full)
    xs = Frame([v for v in full.vecs if v.name in names])
    ens = m.ens
    K, T = int(ens.K), int(ens.ntrees * ens.K)
    top = [r[0] for r in m.varimp()][:2]
    fs, ff = m.x.index(top[0]), m.x.index(top[1])
    Xc = m.adapt_frame(xs).feature_matrix(m.x).float().contiguous()
    n = int(Xc.shape[1])

    def linspace(f):
        return np.linspace(float(Xc[f].min()), float(Xc[f].max()), NBINS).astype(np.float32)

    grid, fixed = linspace(fs), linspace(ff)
    info = {"arm": arm, "rows": n, "trees": T, "columns": top}
    nodes, cbits, roots = ens.device_nodes(dev, T)
    init = torch.from_numpy(ens.init_f.astype(np.float32)).to(dev)
    if arm in "ac":
        Xw = Xc.clone()
        out = torch.empty((K, n), dtype=torch.float32, device=dev)
        lib = tree_lib()
        ys = [None] if arm == "a" else list(fixed)

        def run():
            for fy in ys:
                if fy is not None:
                    Xw[ff] = float(fy)
                for gv in grid:
                    Xw[fs] = float(gv)
                    out.copy_(init[:, None].expand(K, n))
                    check(lib.h2omx_predict_raw(P(Xw), Xw.stride(0), n, P(nodes), P(roots), T, K, P(out),
                                                out.stride(0), P(cbits), stream(dev)), "predict_raw")
        info["launches"] = len(ys) * len(grid)
    elif arm in "bd":
        NY = 1 if arm == "b" else len(fixed)
        thr = np.ascontiguousarray(ens.trees[:T]["thr"]).reshape(-1)
        ub = torch.from_numpy(np.searchsorted(grid, thr, side="right").astype(np.int32)).to(dev)
        gd = torch.from_numpy(grid).to(dev)
        fd = torch.from_numpy(fixed).to(dev) if arm == "d" else None
        out = torch.empty((NY, len(grid), K, n), dtype=torch.float32, device=dev)
        lib = explain_lib()
        walks = torch.zeros(1, dtype=torch.int64, device=dev)

        def run(count=None):
            out.copy_(init[None, None, :, None].expand_as(out))
            check(lib.h2omx_pd_sweep(P(Xc), Xc.stride(0), n, F, P(nodes), P(roots), T, K, P(cbits), fs, P(gd), P(ub),
                                     len(grid), len(grid), ff if arm == "d" else -1, P(fd), NY, P(out), P(count),
                                     stream(dev)), "pd_sweep")
        info["launches"] = 1
    elif arm == "e":
        def run():
            return _loop_partial_dependence(m, xs, top[0], NBINS)
    else:
        def run():
            return m.partial_dependence(xs, [top[0]], nbins=NBINS)[0]

    def timed():
        if arm in "abcd":
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            a.record()
            run()
            b.record()
            torch.cuda.synchronize(dev)
            return a.elapsed_time(b)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = run()
        torch.cuda.synchronize(dev)
        info["first_mean"] = r["data"][0]["mean_response"]
        return (time.perf_counter() - t0) * 1e3

    for _ in range(warmup):
        timed()
    info["ms"] = [timed() for _ in range(repeats)]
    if arm in "bd":
        # the walk count comes from the counting instantiation, outside the timed calls; its margins are compared
        # with one scoring launch on the first cell
        run(walks)
        torch.cuda.synchronize(dev)
        info["walks_per_row_tree"] = float(walks) / (n * T * out.shape[0])
        Xw = Xc.clone()
        Xw[fs] = float(grid[0])
        if arm == "d":
            Xw[ff] = float(fixed[0])
        info["first_cell_equal"] = bool(torch.equal(out[0, 0], ens.raw_margin(Xw)))
    return info


def _fmt(v):
    return f"{statistics.median(v):10.3f}  [{min(v):.3f} .. {max(v):.3f}]"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "partial_dependence.txt"))
    ap.add_argument("--arm", choices=ARMS, help="run one arm in this process and print its JSON line")
    a = ap.parse_args()
    if a.arm:
        print("RESULT " + json.dumps(_arm(a.arm, a.rows, a.warmup, a.repeats)), flush=True)
        return
    res = {}
    for arm in ARMS:                       # a fresh process per arm; the first failure ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--rows", str(a.rows),
                            "--warmup", str(a.warmup), "--repeats", str(a.repeats)],
                           stdout=subprocess.PIPE, text=True, timeout=240)
        if p.returncode != 0:
            raise SystemExit(f"arm {arm} failed with status {p.returncode}")
        res[arm] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(f"arm {arm} done", flush=True)
    r0 = res["a"]
    what = {"a": "20 x h2omx_predict_raw", "b": "h2omx_pd_sweep, 20 cells", "c": "400 x h2omx_predict_raw",
            "d": "h2omx_pd_sweep, 20 x 20 cells", "e": "public 1-D call, loop per cell",
            "f": "public 1-D call, model.partial_dependence"}
    lines = [f"# partial dependence timing: GBM {r0['trees']} trees depth 5, 28 features, {r0['rows']} rows, "
             f"columns {', '.join(r0['columns'])}, {NBINS} grid values each",
             f"# {a.warmup} warm-up + {a.repeats} timed calls per arm, a fresh process per arm; "
             "ms, median [min .. max]",
             "# a - d: device events around the launches; e, f: host clock around the call + synchronise",
             f"{'arm':4s} {'what':42s} {'ms':>34s}  notes"]
    for arm in ARMS:
        r = res[arm]
        note = ""
        if "walks_per_row_tree" in r:
            note = (f"{r['walks_per_row_tree']:.2f} walks per (row, tree), "
                    f"first cell bit-equal to predict_raw: {r['first_cell_equal']}")
        if "first_mean" in r:
            note = f"mean_response of the first cell {r['first_mean']!r}"
        lines.append(f"{arm:4s} {what[arm]:42s} {_fmt(r['ms']):>34s}  {note}")
    for slow, fast in (("a", "b"), ("c", "d"), ("e", "f")):
        s, f = res[slow]["ms"], res[fast]["ms"]
        lines.append(f"{fast} / {slow}: {statistics.median(f) / statistics.median(s):.3f} of the time; ranges "
                     + ("do not overlap" if max(f) < min(s) or max(s) < min(f) else "overlap"))
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt)
    print(txt, end="")


if __name__ == "__main__":
    main()
