"""Time the H statistic's partial-dependence kernel against the path-dependent
SHAP kernel.

One GBM (50 trees, depth 5, 28 features, seeded synthetic data) and 100k rows;
one arm per process:

  shap     the path-dependent SHAP kernel (h2omx_tree_shap), for scale
  k2 k3 k6 h2omx_friedman_h_pd on the 2, 3 and 6 most important features (varimp)

Per arm: warm-up calls, then repeated calls timed twice over: device events
around the native entry point alone (buffers allocated and the leaf table
uploaded once), and a host clock around the public call (``model.h``, for
``shap`` ``predict_contributions``) ending in a synchronise, so path
flattening, the leaf table, uploads and the moment reductions are included.
Reported: median and min-max of the repeats, and the leaves each k keeps.

    python scripts/friedman_h_timing.py --out profiles/r10/friedman_h.txt
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

ARMS = ("shap", "k2", "k3", "k6")


def _arm(arm: str, rows: int, warmup: int, repeats: int) -> dict:
    import numpy as np
    import torch

    from h2omx import explain as ex
    from h2omx.frame import Frame
    from h2omx.models import H2OGradientBoostingEstimator
    from h2omx.ops import P, check, explain_lib, stream

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
    nt = ens.ntrees
    lv, el, _, maxm, sets = ex.tree_paths(ens.trees[:nt], 1.0)
    fr = m.adapt_frame(xs)
    Xc = (m._matrix(fr) if hasattr(m, "_matrix") else fr.feature_matrix(m.x)).float().contiguous()
    n, L = Xc.shape[1], int(lv.shape[0])
    lib = explain_lib()
    info = {"arm": arm, "rows": n, "leaves": L, "maxm": int(maxm)}
    if arm == "shap":
        lvd = torch.from_numpy(lv).to(dev)
        eld = torch.from_numpy(el).to(dev)
        setd = torch.from_numpy(sets.view(np.int32).copy()).to(dev)
        wt = torch.from_numpy(ex.shapley_weights(ex._bucket(maxm)).astype(np.float32)).to(dev)
        out = torch.zeros((F, n), dtype=torch.float32, device=dev)

        def native():
            check(lib.h2omx_tree_shap(P(Xc), Xc.stride(0), n, F, P(lvd), L, P(eld), P(wt), maxm, P(out), P(setd),
                                      stream(dev)), "tree_shap")

        def public():
            return ex.predict_contributions(m, xs)
    else:
        k = int(arm[1:])
        ranked = [r[0] for r in m.varimp()]
        variables = ranked[:k]
        table = ex._h_leaf_table(lv, el, [m.x.index(v) for v in variables])
        kept = int(table["hdr"].shape[0])
        nsub = (1 << k) - 1
        nchunks = ex._h_chunks(n, kept, nsub, torch.cuda.mem_get_info(dev)[0] // 2)
        chunk = -(-kept // nchunks)
        nchunks = -(-kept // chunk)
        hd = torch.from_numpy(table["hdr"]).to(dev)
        wd = torch.from_numpy(table["w"]).to(dev)
        slabs = torch.empty((nchunks, nsub, n), dtype=torch.float64, device=dev) if nchunks > 1 else None
        out = torch.empty((nsub, n), dtype=torch.float64, device=dev)
        v = table["vars"] + [0] * (ex.H_MAX_VARS_DEVICE - k)
        info.update(k=k, variables=variables, kept=kept, chunks=nchunks)

        def native():
            check(lib.h2omx_friedman_h_pd(P(Xc), Xc.stride(0), n, F, k, *v, P(hd), P(wd), kept, chunk, P(slabs),
                                          P(out), stream(dev)), "friedman_h_pd")

        def public():
            return m.h(xs, variables)

    def timed_native():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        native()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b)

    def timed_public():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = public()
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) * 1e3
        if arm != "shap":
            info["h"] = r
        del r
        return dt

    for _ in range(warmup):
        timed_native()
        timed_public()
    info["native_ms"] = [timed_native() for _ in range(repeats)]
    info["public_ms"] = [timed_public() for _ in range(repeats)]
    return info


def _fmt(v):
    return f"{statistics.median(v):10.3f}  [{min(v):.3f} .. {max(v):.3f}]"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "friedman_h.txt"))
    ap.add_argument("--arm", choices=ARMS, help="run one arm in this process and print its JSON line")
    a = ap.parse_args()
    if a.arm:
        print("RESULT " + json.dumps(_arm(a.arm, a.rows, a.warmup, a.repeats)), flush=True)
        return
    res = {}
    for arm in ARMS:                       # a fresh process per arm
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--rows", str(a.rows),
                            "--warmup", str(a.warmup), "--repeats", str(a.repeats)],
                           stdout=subprocess.PIPE, text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit(f"arm {arm} failed with status {p.returncode}")
        res[arm] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    r0 = res["shap"]
    lines = [f"# H statistic timing: GBM 50 trees depth 5, 28 features, {r0['rows']} rows, {r0['leaves']} leaves "
             f"(max {r0['maxm']} features a path)",
             f"# {a.warmup} warm-up + {a.repeats} timed calls per arm, a fresh process per arm; "
             "ms, median [min .. max]",
             "# native = device events around the entry point; public = model.h (shap: predict_contributions) "
             "+ synchronise",
             f"{'arm':6s} {'kept':>5s} {'chunks':>6s}  {'native ms':>34s}  {'public ms':>34s}  h"]
    for arm in ARMS:
        r = res[arm]
        lines.append(f"{arm:6s} {r.get('kept', r['leaves']):5d} {r.get('chunks', 1):6d}  {_fmt(r['native_ms']):>34s}  "
                     f"{_fmt(r['public_ms']):>34s}  "
                     + (f"{r['h']:.4f} {','.join(r['variables'])}" if "h" in r else "-"))
    base = statistics.median(r0["native_ms"])
    for arm in ARMS[1:]:
        t = statistics.median(res[arm]["native_ms"])
        lines.append(f"{arm}: {t / base:.3f} x the path-dependent SHAP kernel's {base:.3f} ms")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt)
    print(txt, end="")


if __name__ == "__main__":
    main()
