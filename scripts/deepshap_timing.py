"""Time the DeepSHAP stages of ``predict_contributions`` for a Deep Learning
model: hidden = [200, 200], 28 numerical predictors, 1000 scored rows against
100 background rows (100k pairs, [100000][200] float32 planes of 80 MB).

One arm per process:

  torch_rescale  U = G * r(zx, zb) as torch elementwise ops in float32 (the same
                 closed forms, h2omx.explain._deepshap_multiplier), per
                 activation; checked equal to the kernel before it is timed
  rescale        h2omx_deepshap_rescale per activation, G a plane (reads G,
                 writes U: 160 MB) and G the top layer's vector (writes 80 MB)
  copy           the simplest stream of the same 160 MB: Tensor.copy_ of a plane
  gemm           the two GEMMs of the backward pass, [100000][200] x [200][200]
                 and [100000][200] x [200][28] (ops.dense.gemm)
  fold           h2omx_deepshap_fold, per pair and background mean
  torch_fold     the same two results as one torch expression each; checked
                 equal to the kernel before it is timed
  public         model.predict_contributions(frame, background_frame=..) in both
                 forms, wall time ending in a synchronise

Per arm: warm-up calls, then repeated calls with device events around the
launches (``public``: a host clock).  Reported: median and min .. max.

    python scripts/deepshap_timing.py --out profiles/r16/deepshap.txt
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

ARMS = ("torch_rescale", "rescale", "copy", "gemm", "fold", "torch_fold", "public")
ACTS = {"Rectifier": 1, "Tanh": 2, "ExpRectifier": 4}
N, NB, H, F = 1000, 100, 200, 28


def _arm(arm: str, warmup: int, repeats: int) -> dict:
    import torch

    from h2omx import explain as ex
    from h2omx.frame import Frame
    from h2omx.models import H2ODeepLearningEstimator
    from h2omx.ops import P, check, explain_lib, stream
    from h2omx.ops import dense as OD

    dev = torch.device("cuda", 0)
    lib, st = explain_lib(), stream(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    info = {"arm": arm, "ms": {}}
    pairs = N * NB

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

    def close(a, b, what):
        tol = 2e-4 * max(1.0, float(b.abs().max()))
        err = float((a - b).abs().max())
        if not err <= tol:
            raise SystemExit(f"{what}: the torch expression differs from the kernel by {err:.3e} (tolerance {tol:.3e})")
        return err

    if arm == "public":
        X = torch.randn((2000 + N + NB, F), generator=g, device=dev)
        y = X[:, 0] - X[:, 1] * X[:, 2] + 0.3 * torch.randn(X.shape[0], generator=g, device=dev)
        full = Frame.from_tensor(X[:2000].t().contiguous(), y=y[:2000])
        names = full.names[:-1]
        m = H2ODeepLearningEstimator(hidden=[H, H], epochs=1, seed=1).train(y=full.names[-1], training_frame=full)
        xs = Frame.from_tensor(X[2000:2000 + N].t().contiguous(), names=names)
        bs = Frame.from_tensor(X[2000 + N:].t().contiguous(), names=names)
        info["ms"]["averaged"] = series(wall, lambda: m.predict_contributions(xs, background_frame=bs))
        info["ms"]["per_reference"] = series(wall, lambda: m.predict_contributions(xs, background_frame=bs,
                                                                                  output_per_reference=True))
        return info
    # synthetic operands of the stages: pre-activations of both signs, O(1) multipliers
    Zx = torch.randn((N, H), generator=g, device=dev)
    Zb = torch.randn((NB, H), generator=g, device=dev)
    G = torch.randn((pairs, H), generator=g, device=dev)
    gv = torch.randn((H,), generator=g, device=dev)
    U = torch.empty_like(G)

    def rescale(act, vec):
        check(lib.h2omx_deepshap_rescale(P(gv if vec else G), int(vec), P(Zx), P(Zb), P(U), N, NB, H, act, st),
              "deepshap_rescale")

    def torch_rescale(act, vec):
        r = ex._deepshap_multiplier(act, Zx[:, None, :], Zb[None, :, :])
        return ((gv if vec else G.view(N, NB, H)) * r).view(pairs, H)

    if arm in ("rescale", "torch_rescale"):
        for name, act in ACTS.items():
            for vec in (False, True):
                key = f"{name} {'vector' if vec else 'plane'}"
                rescale(act, vec)
                info.setdefault("err", {})[key] = close(torch_rescale(act, vec), U, key)
                fn = (lambda: rescale(act, vec)) if arm == "rescale" else (lambda: torch_rescale(act, vec))
                info["ms"][key] = series(events, fn)
        return info
    if arm == "copy":
        info["ms"]["copy_ 80 MB -> 80 MB"] = series(events, lambda: U.copy_(G))
        return info
    if arm == "gemm":
        W1 = torch.randn((H, H), generator=g, device=dev) / H ** 0.5
        W0 = torch.randn((H, F), generator=g, device=dev) / H ** 0.5
        o1, o0 = torch.empty((pairs, H), device=dev), torch.empty((pairs, F), device=dev)
        info["ms"][f"[{pairs}][{H}] x [{H}][{H}]"] = series(events, lambda: OD.gemm(G, W1, out=o1))
        info["ms"][f"[{pairs}][{H}] x [{H}][{F}]"] = series(events, lambda: OD.gemm(G, W0, out=o0))
        return info
    G0 = torch.randn((pairs, F), generator=g, device=dev)
    xs = torch.randn((N, F), generator=g, device=dev)
    bs = torch.randn((NB, F), generator=g, device=dev)
    cs = torch.arange(F + 1, dtype=torch.int32, device=dev)
    scale = 1.7
    outs = {False: torch.empty((F, pairs), device=dev), True: torch.empty((F, N), device=dev)}

    def fold(mean):
        o = outs[mean]
        check(lib.h2omx_deepshap_fold(P(G0), P(xs), P(bs), P(cs), scale, N, NB, F, F, int(mean), int(o.shape[1]), P(o),
                                      st), "deepshap_fold")

    def torch_fold(mean):
        phi = scale * G0.view(N, NB, F) * (xs[:, None, :] - bs[None, :, :])
        return (phi.sum(1) / NB).t().contiguous() if mean else phi.view(pairs, F).t().contiguous()

    for mean in (False, True):
        key = "background mean" if mean else "per pair"
        fold(mean)
        info.setdefault("err", {})[key] = close(torch_fold(mean), outs[mean], key)
        info["ms"][key] = series(events, (lambda: fold(mean)) if arm == "fold" else (lambda: torch_fold(mean)))
    return info


def _fmt(v):
    return f"{statistics.median(v):10.3f}  [{min(v):.3f} .. {max(v):.3f}]"


def _versus(lines, what, torch_ms, kernel_ms):
    tm, km = statistics.median(torch_ms), statistics.median(kernel_ms)
    spread = max(max(torch_ms) - min(torch_ms), max(kernel_ms) - min(kernel_ms))
    lines.append(f"{what}: kernel {km:.3f} ms, torch {tm:.3f} ms ({tm / km:.1f} x); the kernel is "
                 f"{'faster by more' if tm - km > spread else 'NOT faster by more'} than the larger min .. max spread "
                 f"({spread:.3f} ms)")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "deepshap.txt"))
    ap.add_argument("--arm", choices=ARMS, help="run one arm in this process")
    a = ap.parse_args()
    if a.arm:
        print("RESULT " + json.dumps(_arm(a.arm, a.warmup, a.repeats)), flush=True)
        return
    res = {}
    for arm in ARMS:                                  # a fresh process per arm, each under its own time limit
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--warmup", str(a.warmup),
                            "--repeats", str(a.repeats)], stdout=subprocess.PIPE, text=True, timeout=240)
        if p.returncode != 0:
            raise SystemExit(f"arm {arm} failed with status {p.returncode}")
        res[arm] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    plane = N * NB * H * 4
    lines = ["# DeepSHAP stages: hidden [200, 200], 28 predictors, 1000 scored x 100 background rows (100000 pairs)",
             f"# {a.warmup} warm-up + {a.repeats} timed calls per arm, a fresh process per arm; ms, median [min .. max]",
             "# stages: device events around the launches; public: host clock + synchronise"]
    for arm in ARMS:
        for name, v in res[arm]["ms"].items():
            lines.append(f"{arm:14s} {name:28s} {_fmt(v):>40s}")
    for key, e in res["torch_rescale"]["err"].items():
        lines.append(f"max |torch - kernel| rescale {key}: {e:.3e}")
    for key, e in res["torch_fold"]["err"].items():
        lines.append(f"max |torch - kernel| fold {key}: {e:.3e}")
    for key in res["rescale"]["ms"]:
        _versus(lines, f"rescale {key}", res["torch_rescale"]["ms"][key], res["rescale"]["ms"][key])
    for key in res["fold"]["ms"]:
        _versus(lines, f"fold {key}", res["torch_fold"]["ms"][key], res["fold"]["ms"][key])
    cp = statistics.median(next(iter(res["copy"]["ms"].values())))
    lines.append(f"stream: copy_ moves {2 * plane / cp / 1e9:.2f} TB/s (read + write)")
    for key, v in res["rescale"]["ms"].items():
        moved = plane if key.endswith("vector") else 2 * plane
        lines.append(f"stream: rescale {key} moves {moved / statistics.median(v) / 1e9:.2f} TB/s "
                     f"({moved / statistics.median(v) / (2 * plane / cp) * 100:.0f} % of the copy's rate)")
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt)
    print(txt, end="")


if __name__ == "__main__":
    main()
