"""Time the path-dependent TreeSHAP entry point (h2omx_tree_shap) alone, with
the libraries of two builds: this tree's and another's (the parent commit's,
built in a second checkout and named by --parent-lib-dir).

Two shapes, each arm in a fresh process:

  depth8   one GBM (50 trees, depth 8, 28 features, seeded synthetic data)
           scored on 100k rows: the MAXM = 8 instantiation, all in fp32
  wide32   the near-one 32-wide synthetic path table of tests/shapref.py
           (31 leaves of up to 32 features, F = 40) with its 300 rows tiled to
           100k: the MAXM = 32 instantiation

Per arm: warm-up calls, then repeated calls between device events (buffers
allocated once, the output zeroed outside the timed span).  Reported: median
and min-max of the repeats.

    python scripts/tree_shap_timing.py --parent-lib-dir ../parent/h2omx/lib \\
        --out profiles/r13/tree_shap.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("depth8", "wide32")


def _arm(shape: str, rows: int, warmup: int, repeats: int) -> dict:
    import numpy as np
    import torch

    from h2omx import _native
    from h2omx import explain as ex
    from h2omx.ops import P, check, explain_lib, stream

    dev = torch.device("cuda", 0)
    if shape == "depth8":
        from h2omx.frame import Frame
        from h2omx.models import H2OGradientBoostingEstimator

        F = 28
        g = torch.Generator(device=dev).manual_seed(7)
        X = torch.randn((rows, F), generator=g, device=dev)
        y = ((X[:, 0] + X[:, 1] * X[:, 2] - 0.5 * X[:, 3] + torch.randn(rows, generator=g, device=dev)) > 0).float()
        full = Frame.from_tensor(X.t().contiguous(), y=y, y_categorical=True)
        full.vecs[-1].domain = ["0", "1"]
        m = H2OGradientBoostingEstimator(ntrees=50, max_depth=8, seed=1).train(y=full.names[-1], training_frame=full)
        lv, el, _, maxm, sets = ex.tree_paths(m.ens.trees[: m.ens.ntrees], 1.0)
        Xc = X.t().contiguous()
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import shapref

        t = shapref.tables(32, "near_one", 40)
        lv, el, maxm, sets = t["lv"], t["el"], t["maxm"], t["sets"]
        F = t["X"].shape[0]
        Xc = torch.from_numpy(np.tile(t["X"], (1, -(-rows // t["X"].shape[1])))[:, :rows].copy()).to(dev)
    n, L = int(Xc.shape[1]), int(lv.shape[0])
    lvd = torch.from_numpy(np.ascontiguousarray(lv, np.int32)).to(dev)
    eld = torch.from_numpy(el).to(dev)
    setd = torch.from_numpy(sets.view(np.int32).copy()).to(dev)
    wt = torch.from_numpy(ex.shapley_weights(ex._bucket(maxm)).astype(np.float32)).to(dev)
    out = torch.zeros((F, n), dtype=torch.float32, device=dev)
    lib = explain_lib()

    def timed():
        out.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        check(lib.h2omx_tree_shap(P(Xc), Xc.stride(0), n, F, P(lvd), L, P(eld), P(wt), maxm, P(out), P(setd),
                                  stream(dev)), "tree_shap")
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b)

    for _ in range(warmup):
        timed()
    ms = [timed() for _ in range(repeats)]
    return {"shape": shape, "rows": n, "F": F, "leaves": L, "maxm": int(maxm), "bucket": ex._bucket(maxm), "ms": ms,
            "checksum": float(out.double().abs().sum()), "lib": _native.lib_path("explain")}


def _fmt(v):
    return f"{statistics.median(v):10.3f}  [{min(v):.3f} .. {max(v):.3f}]"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--parent-lib-dir", help="libraries built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "tree_shap.txt"))
    ap.add_argument("--shape", choices=SHAPES, help="run one arm in this process and print its JSON line")
    a = ap.parse_args()
    if a.shape:
        print("RESULT " + json.dumps(_arm(a.shape, a.rows, a.warmup, a.repeats)), flush=True)
        return
    if not a.parent_lib_dir:
        ap.error("--parent-lib-dir is required")
    res = {}
    for build, libdir in (("parent", os.path.abspath(a.parent_lib_dir)), ("this", None)):
        for shape in SHAPES:                       # a fresh process per arm
            env = dict(os.environ)
            env.pop("H2OMX_LIB_DIR", None)
            if libdir:
                env["H2OMX_LIB_DIR"] = libdir
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", shape, "--rows", str(a.rows),
                                "--warmup", str(a.warmup), "--repeats", str(a.repeats)],
                               stdout=subprocess.PIPE, text=True, timeout=600, env=env)
            if p.returncode != 0:
                raise SystemExit(f"arm {build}/{shape} failed with status {p.returncode}")
            res[build, shape] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    lines = [f"# h2omx_tree_shap alone, device events; {a.warmup} warm-up + {a.repeats} timed calls per arm, a fresh "
             "process per arm; ms, median [min .. max]",
             "# parent = the libraries of the parent commit (fp32 at every width); this = MAXM = 32 in fp64"]
    for shape in SHAPES:
        r = res["this", shape]
        lines.append(f"# {shape}: {r['rows']} rows, F = {r['F']}, {r['leaves']} leaves, up to {r['maxm']} features a "
                     f"path (MAXM = {r['bucket']})")
    lines.append(f"{'shape':8s} {'build':8s} {'ms':>34s}  {'sum |phi|':>16s}")
    for shape in SHAPES:
        for build in ("parent", "this"):
            r = res[build, shape]
            lines.append(f"{shape:8s} {build:8s} {_fmt(r['ms']):>34s}  {r['checksum']:16.6f}")
        t0, t1 = (statistics.median(res[b, shape]["ms"]) for b in ("parent", "this"))
        lines.append(f"{shape}: this / parent = {t1 / t0:.3f}")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt)
    print(txt, end="")


if __name__ == "__main__":
    main()
