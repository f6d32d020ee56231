"""Time the interventional SHAP kernels against the path-dependent one.

One GBM (50 trees, depth 5, 28 features, seeded synthetic data) and 100k
scored rows; three arms, each in a fresh process:

  path     the existing path-dependent kernel (h2omx_tree_shap)
  avg      h2omx_tree_shap_background, nb = 100, averaged over the background
  perref   the same entry point with chunk 1 (one slab per background row)

Per arm: warm-up calls, then repeated calls timed twice over: device events
around the native entry point alone (buffers allocated once), and a host
clock around the public predict_contributions call ending in a synchronise
(path table flattening, uploads, slab zeroing and the per-reference
transpose included).  Reported: median and min-max of the repeats.

    python scripts/shap_background_timing.py --out profiles/r9/shap_background.txt
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

ARMS = ("path", "avg", "perref")


def _arm(arm: str, rows: int, nb: int, warmup: int, repeats: int) -> dict:
    import numpy as np
    import torch

    from h2omx import explain as ex
    from h2omx.frame import Frame
    from h2omx.models import H2OGradientBoostingEstimator
    from h2omx.ops import P, check, explain_lib, stream

    dev = torch.device("cuda", 0)
    F = 28
    g = torch.Generator(device=dev).manual_seed(7)
    X = torch.randn((rows + nb, F), generator=g, device=dev)
    y = ((X[:, 0] + X[:, 1] * X[:, 2] - 0.5 * X[:, 3] + torch.randn(rows + nb, generator=g, device=dev)) > 0).float()
    full = Frame.from_tensor(X.t().contiguous(), y=y, y_categorical=True)
    full.vecs[-1].domain = ["0", "1"]
    names = full.names[:-1]
    m = H2OGradientBoostingEstimator(ntrees=50, max_depth=5, seed=1).train(y=full.names[-1], training_frame=full)
    xs = Frame([v for v in full.rows(torch.arange(rows, device=dev)).vecs if v.name in names])
    xb = Frame([v for v in full.rows(torch.arange(rows, rows + nb, device=dev)).vecs if v.name in names])
    ens = m.ens
    nt = ens.ntrees
    lv, el, _, maxm, sets = ex.tree_paths(ens.trees[:nt], 1.0)
    Xc = m._matrix(m.adapt_frame(xs)).float().contiguous() if hasattr(m, "_matrix") else \
        m.adapt_frame(xs).feature_matrix(m.x).float().contiguous()
    Bc = m._matrix(m.adapt_frame(xb)).float().contiguous() if hasattr(m, "_matrix") else \
        m.adapt_frame(xb).feature_matrix(m.x).float().contiguous()
    n, L = Xc.shape[1], int(lv.shape[0])
    lvd = torch.from_numpy(lv).to(dev)
    eld = torch.from_numpy(el).to(dev)
    setd = torch.from_numpy(sets.view(np.int32).copy()).to(dev)
    lib = explain_lib()
    if arm == "path":
        wt = torch.from_numpy(ex.shapley_weights(ex._bucket(maxm)).astype(np.float32)).to(dev)
        out = torch.zeros((F, n), dtype=torch.float32, device=dev)

        def native():
            out.zero_()
            return lambda: check(lib.h2omx_tree_shap(P(Xc), Xc.stride(0), n, F, P(lvd), L, P(eld), P(wt), maxm, P(out),
                                                     P(setd), stream(dev)), "tree_shap")

        def public():
            return ex.predict_contributions(m, xs)
        chunk = nslabs = 0
    else:
        per = arm == "perref"
        wt = torch.from_numpy(ex.baseline_weights().astype(np.float32)).to(dev)
        chunk = 1 if per else ex._background_chunk(n, nb, F, torch.cuda.mem_get_info(dev)[0] // 2)
        nslabs = -(-nb // chunk)
        bmask = torch.empty((L, nb), dtype=torch.int32, device=dev)
        slabs = torch.zeros((nslabs, F, n), dtype=torch.float32, device=dev)
        out = None if per else torch.empty((F, n), dtype=torch.float32, device=dev)
        lds = F * 256 * 4 <= 64 * 1024

        def native():
            if not lds:
                slabs.zero_()          # the global-accumulator path adds into the slabs
            return lambda: check(lib.h2omx_tree_shap_background(
                P(Xc), Xc.stride(0), n, F, P(Bc), Bc.stride(0), nb, P(lvd), L, P(eld), P(wt), maxm, P(setd),
                P(bmask), chunk, P(slabs), P(out), stream(dev)), "tree_shap_background")

        def public():
            return ex.predict_contributions(m, xs, background_frame=xb, output_per_reference=per)

    def timed_native():
        call = native()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b)

    def timed_public():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = public()
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) * 1e3
        del r
        return dt

    for _ in range(warmup):
        timed_native()
        timed_public()
    nat = [timed_native() for _ in range(repeats)]
    pub = [timed_public() for _ in range(repeats)]
    return {"arm": arm, "rows": n, "nb": nb if arm != "path" else 0, "leaves": L, "maxm": int(maxm),
            "chunk": chunk, "slabs": nslabs, "native_ms": nat, "public_ms": pub}


def _fmt(v):
    return f"{statistics.median(v):10.3f}  [{min(v):.3f} .. {max(v):.3f}]"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--nb", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r9", "shap_background.txt"))
    ap.add_argument("--arm", choices=ARMS, help="run one arm in this process and print its JSON line")
    a = ap.parse_args()
    if a.arm:
        print("RESULT " + json.dumps(_arm(a.arm, a.rows, a.nb, a.warmup, a.repeats)), flush=True)
        return
    res = {}
    for arm in ARMS:                       # a fresh process per arm
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--rows", str(a.rows), "--nb",
                            str(a.nb), "--warmup", str(a.warmup), "--repeats", str(a.repeats)],
                           stdout=subprocess.PIPE, text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit(f"arm {arm} failed with status {p.returncode}")
        res[arm] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    r0 = res["path"]
    lines = [f"# interventional SHAP timing: GBM 50 trees depth 5, 28 features, {r0['rows']} scored rows, "
             f"{r0['leaves']} leaves (max {r0['maxm']} features a path), nb = {a.nb}",
             f"# {a.warmup} warm-up + {a.repeats} timed calls per arm, a fresh process per arm; "
             "ms, median [min .. max]",
             "# native = device events around the entry point; public = predict_contributions + synchronise",
             f"{'arm':8s} {'slabs':>5s}  {'native ms':>34s}  {'public ms':>34s}"]
    for arm in ARMS:
        r = res[arm]
        lines.append(f"{arm:8s} {r['slabs']:5d}  {_fmt(r['native_ms']):>34s}  {_fmt(r['public_ms']):>34s}")
    base = statistics.median(r0["native_ms"])
    for arm in ("avg", "perref"):
        t = statistics.median(res[arm]["native_ms"])
        lines.append(f"{arm}: {t / a.nb:.4f} ms per background row = {t / a.nb / base:.3f} x the path-dependent "
                     f"kernel's {base:.3f} ms")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt)
    print(txt, end="")


if __name__ == "__main__":
    main()
