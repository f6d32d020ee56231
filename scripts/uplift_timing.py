"""Uplift DRF: the tensor route against the ops.uplift kernels, phase by phase and whole.

    python scripts/uplift_timing.py [--out profiles/r22/uplift.txt] [--small] [--arms a,b,...]

Protocol: medians of 7 after 2 warm-ups with min .. max, a fresh process per arm, device
events around the calls, next to the same process's Tensor.copy_ rate.  Data: 1M x 20
standard normal columns, nbins 20, a treatment effect on the first column.
Arms ``<phase>_<torch|hip>`` on the same inputs:
  hist1 / hist128 / hist2048   one level's histogram with that many build slots (level 0;
                               a deep level on the LDS path; one on the global path), half
                               of the bagged rows in a built child
  split256                     the split scan of 256 nodes, KL
  route256                     routing 256 nodes' rows and forming the next keys
  predictA / predictB          _predict_raw_torch against predict_raw
  fitA / fitB                  the public fit with tree_engine forced either way
A: 10 trees, depth 10.  B: the defaults, 50 trees, depth 20.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PHASES = ["hist1", "hist128", "hist2048", "split256", "route256", "predictA", "predictB", "fitA", "fitB"]
ARMS = [f"{p}_{r}" for p in PHASES for r in ("torch", "hip")]
REPS, WARM = 7, 2
SHAPES = {"A": dict(ntrees=10, max_depth=10), "B": dict(ntrees=50, max_depth=20)}


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


def _split_torch(Hc, fmask, bin_ok, metric, min_rows):
    """The split scan of _grow_torch on fp64 counts [K][F][nbt][4]."""
    import torch

    from h2omx.models.uplift import _ratio, divergence

    K, F, nbt, _ = Hc.shape
    dev = Hc.device
    H = torch.stack([Hc[..., 0] + Hc[..., 1], Hc[..., 1], Hc[..., 2] + Hc[..., 3], Hc[..., 3]])
    na = H[..., nbt - 1]
    cum = torch.cumsum(H[..., : nbt - 1], -1)
    node_tot = H[:, :, 0, :].sum(-1)
    T = node_tot[:, :, None, None]
    zero = torch.zeros(K, dtype=torch.float64, device=dev)
    pn = _ratio(node_tot[1], node_tot[0], zero)
    qn = _ratio(node_tot[3], node_tot[2], zero)
    d_node = divergence(pn, qn, metric)
    ntot = (node_tot[0] + node_tot[2]).clamp_min(1e-300)
    best_gain = torch.full((K,), -math.inf, dtype=torch.float64, device=dev)
    best = torch.zeros((K, 3), dtype=torch.long, device=dev)
    for na_left in (0, 1):
        L = cum + (na[..., None] if na_left else 0.0)
        R = T - L
        nL, nR = L[0] + L[2], R[0] + R[2]
        valid = ((nL >= min_rows) & (nR >= min_rows) & (L[0] > 0) & (L[2] > 0) & (R[0] > 0) & (R[2] > 0)
                 & bin_ok[None] & fmask[:, :, None])
        dL = divergence(_ratio(L[1], L[0], pn[:, None, None]), _ratio(L[3], L[2], qn[:, None, None]), metric)
        dR = divergence(_ratio(R[1], R[0], pn[:, None, None]), _ratio(R[3], R[2], qn[:, None, None]), metric)
        gain = (nL * dL + nR * dR) / ntot[:, None, None] - d_node[:, None, None]
        gain = torch.where(valid, gain, torch.full_like(gain, -math.inf))
        gv, gi = gain.view(K, -1).max(1)
        upd = gv > best_gain
        best_gain = torch.where(upd, gv, best_gain)
        fb = torch.stack([gi // (nbt - 1), gi % (nbt - 1), torch.full_like(gi, na_left)], 1)
        best = torch.where(upd[:, None], fb, best)
    kk = torch.arange(K, device=dev)
    Lk = cum[:, kk, best[:, 0], best[:, 1]] + na[:, kk, best[:, 0]] * best[:, 2][None, :]
    return best_gain.cpu(), best.cpu(), Lk.cpu(), node_tot.cpu()


def _route_torch(codes, nid, best, remap_d, br, nbt):
    """The routing expressions of _grow_torch (nid, best, br int64)."""
    import torch

    nid = nid.clone()
    rows = torch.nonzero(nid >= 0).flatten()
    k = nid[rows]
    rk = remap_d[k]
    c = codes[best[k, 0], rows].long()
    right = torch.where(c == nbt - 1, best[k, 2] == 0, c > best[k, 1])
    nid[rows] = torch.where(rk >= 0, 2 * rk + right.long(), torch.full_like(rk, -1))
    return nid, torch.where((nid >= 0) & ((nid & 1) == br[(nid >> 1).clamp_min(0)]), nid >> 1, torch.full_like(nid, -1))


def run_arm(arm: str, small: bool) -> dict:
    import torch

    from h2omx.frame.frame import ENUM, Frame, Vec
    from h2omx.models import H2OUpliftRandomForestEstimator as Est
    from h2omx.models.tree import bin_matrix, compute_edges
    from h2omx.ops import uplift as ops

    dev = torch.device("cuda", 0)
    res = {"arm": arm, "copy_TBps": _copy_rate(dev)}
    phase, side = arm.split("_")
    hip = side == "hip"
    n, F = (100_000 if small else 1_000_000), 20
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn((F, n), generator=g, device=dev)
    t = (torch.rand(n, generator=g, device=dev) < 0.5).float()
    p = (torch.sigmoid(X[1] * 0.5) * 0.6 + t * torch.where(X[0] > 0, 0.3, -0.1)).clamp(0.02, 0.98)
    y = (torch.rand(n, generator=g, device=dev) < p).int()
    if phase.startswith(("fit", "predict")):
        fr = Frame([Vec(f"x{j}", X[j], "real") for j in range(F)]
                   + [Vec("treatment", t.int(), ENUM, ["control", "treatment"]), Vec("y", y, ENUM, ["0", "1"])])
        kw = dict(seed=1, treatment_column="treatment", **SHAPES[phase[-1]])
        if phase.startswith("fit"):
            Est.tree_engine = lambda self, codes: side
            fn = lambda: Est(**kw).train(y="y", training_frame=fr)
        else:
            m = Est(**kw).train(y="y", training_frame=fr)
            res["nodes"] = [int(sum(len(tr["feat"]) for tr in m.trees)), int(max(len(tr["feat"]) for tr in m.trees))]
            fn = (lambda: m.predict_raw(fr)) if hip else (lambda: m._predict_raw_torch(fr))
    else:
        edges, nvb, nbt = compute_edges(X, 20, seed=1)
        codes = bin_matrix(X, edges, nvb, nbt).codes[:, :n]
        S = int(re.sub(r"\D", "", phase))
        rc = ((1 - t) * 2 + y).long()
        rc[torch.rand(n, generator=g, device=dev) >= 0.632] = -1
        node = torch.randint(0, S, (n,), generator=g, device=dev)
        half = torch.rand(n, generator=g, device=dev) < (1.0 if S == 1 else 0.5)
        slot = torch.where((rc >= 0) & half, node, torch.full_like(node, -1))
        key = torch.where(slot >= 0, slot * 4 + rc, torch.full_like(rc, -1)).to(torch.int32)
        res.update(S=S, nbt=nbt)
        if phase.startswith("hist"):
            res["lds"] = ops.hist_lds(S, nbt)
            fn = (lambda: ops.category_hist(codes, key, S, nbt)) if hip else \
                (lambda: Est._hist_torch(codes, rc, slot, S, F, nbt, None))
        else:
            Hi = ops.category_hist(codes, key, S, nbt)
            fmask = torch.ones((S, F), dtype=torch.bool, device=dev)
            nvb_d = torch.as_tensor(nvb, dtype=torch.int32, device=dev)
            bin_ok = torch.arange(nbt - 1, device=dev)[None, :] < nvb_d[:, None] - 1
            rec_d = ops.best_splits(Hi, fmask, nvb_d, "KL", 10.0)
            if phase.startswith("split"):
                Hd = Hi.double()
                fn = (lambda: ops.split_records(ops.best_splits(Hi, fmask, nvb_d, "KL", 10.0))) if hip else \
                    (lambda: _split_torch(Hd, fmask, bin_ok, "KL", 10.0))
            else:
                nid = torch.where(rc >= 0, node, torch.full_like(node, -1))
                remap = torch.arange(S, device=dev)
                br = torch.randint(0, 2, (S,), generator=g, device=dev)
                best = rec_d[:, 2:5].long()
                nid32, cat, remap32, br32 = nid.int(), rc.int(), remap.int(), br.int()
                fn = (lambda: ops.route(codes, nid32.clone(), cat, rec_d, remap32, br32, nbt)) if hip else \
                    (lambda: _route_torch(codes, nid, best, remap, br, nbt))
    torch.cuda.synchronize()
    ts = _events(fn)
    res.update(shape=[n, F], median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=ARMS)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "uplift.txt"))
    a = ap.parse_args(argv)
    if a.arm:
        print(json.dumps(run_arm(a.arm, a.small)))
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for arm in a.arms.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm] + (["--small"] if a.small else [])
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            except subprocess.TimeoutExpired:
                print(f"{arm}: not finished in 900 s", file=sys.stderr)
                return 1
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
