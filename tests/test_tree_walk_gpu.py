"""ops.walk (csrc/walk_kernels.hip) against a plain numpy walk of the TREE_NODE_DTYPE records,
one row at a time per tree with float64 sums; every comparison is ``==``.  The staged values
are a fixed sequence of correctly rounded fp64 additions, one fp64 division and one rounding
to fp32, which numpy and the device both do exactly.  The public methods on a device frame are
held to the per-tree tensor bodies they replace."""
from __future__ import annotations

import functools

import numpy as np
import pandas as pd
import pytest
import torch

from h2omx.frame import Frame
from h2omx.models.tree.boost import TreeEnsemble
from h2omx.models.tree.structs import TREE_NODE_DTYPE

pytestmark = pytest.mark.gpu
CODES = np.array([-1, 0, 255, 256, 300], np.float32)
DEPTHS = (1, 4, 4, 4, 4, 11)     # 3 nodes; leaves at mixed depths; 4095 nodes


@functools.lru_cache(maxsize=None)
def _case(n: int, F: int):
    """Matrix, heap-ordered trees and the oracle's ids [T][n] and counts [F][n].  Feature 0 holds
    category codes and splits by group half the time; numbers come from a grid of 7 values and
    every thr is a cell of the matrix, so rows sit exactly on thresholds; 10 % NaN."""
    rng = np.random.default_rng(1000 * n + F)
    X = (rng.integers(-3, 4, (F, n)) / 2).astype(np.float32)
    X[0] = np.where(rng.random(n) < 0.5, rng.choice(CODES, n), rng.integers(0, 256, n))
    X[0, :5] = CODES[:n]
    T, cap = len(DEPTHS), (2 << max(DEPTHS)) - 1
    trees = np.zeros((T, cap), TREE_NODE_DTYPE)
    trees["feat"] = -1
    catbits = np.zeros((T, cap, 8), np.uint32)
    for t, D in enumerate(DEPTHS):
        m = (1 << D) - 1
        tr = trees[t]
        tr["feat"][:m] = rng.integers(0, F, m)
        if D == 4:
            tr["feat"][1:m][rng.random(m - 1) < 0.25] = -1          # subtrees cut to leaves
        tr["thr"][:m] = X[np.maximum(tr["feat"][:m], 0), rng.integers(0, n, m)]
        tr["left"][:m] = 2 * np.arange(m) + 1
        tr["na_left"][:m] = rng.integers(0, 2, m) | np.where((tr["feat"][:m] == 0) & (rng.random(m) < 0.5), 2, 0)
        tr["value"] = rng.normal(size=cap).astype(np.float32)
        catbits[t, :m] = rng.integers(0, 1 << 32, (m, 8), dtype=np.uint64).astype(np.uint32)
    X[rng.random((F, n)) < 0.1] = np.nan
    ids, cnt = np.zeros((T, n), np.int32), np.zeros((F, n), np.float32)
    for t in range(T):
        feat, thr, left, nl = (trees[t][k].tolist() for k in ("feat", "thr", "left", "na_left"))
        for r in range(n):
            i = 0
            for _ in range(64):
                f = feat[i]
                if f < 0:
                    break
                v = X[f, r]
                if v != v:
                    go_left = nl[i] & 1
                elif nl[i] & 2:
                    c = int(v)
                    go_left = (int(catbits[t, i, c >> 5]) >> (c & 31)) & 1 if 0 <= c <= 255 else nl[i] & 1
                else:
                    go_left = v <= np.float32(thr[i])
                cnt[f, r] += 1
                i = left[i] + (0 if go_left else 1)
            ids[t, r] = i
    return X, trees, catbits, ids, cnt


def _ens(trees, catbits, K, average):
    init_f = np.zeros(K) if average else np.linspace(-0.7, 0.9, K)
    return TreeEnsemble(trees=trees, K=K, dist="drf" if average else "multinomial", init_f=init_f, average=average,
                        catbits=catbits)


@pytest.mark.parametrize("K,slab", [(1, None), (3, 1), (1, 3)])
@pytest.mark.parametrize("F", [1, 5, 33, 70])
@pytest.mark.parametrize("n", [1, 257, 600])
def test_ops_against_numpy_walk(cuda_dev, n, F, K, slab):
    from h2omx.ops import walk

    assert 5 <= walk.WALK_XLDS_MAX_F < 33      # the cases straddle the limit of the matrix and counter stage
    X, trees, catbits, ids_ref, cnt_ref = _case(n, F)
    Xd = torch.from_numpy(X).to(cuda_dev)
    for average in (False, True):
        ens = _ens(trees, catbits, K, average)
        plan = walk.pack_walk(ens, cuda_dev)
        used = plan.used.cpu().tolist()
        assert used[0] == 3 and max(used[1:5]) <= 31 and used[5] == 4095
        acc = np.tile(ens.init_f.astype(np.float64)[:, None], (1, n))
        want = np.zeros((plan.T // K, K, n), np.float32)
        for t in range(plan.T):
            acc[t % K] += trees[t]["value"][ids_ref[t]].astype(np.float64)
            want[t // K, t % K] = (acc[t % K] / (t // K + 1)) if average else acc[t % K]
        runs = [(walk.leaf_ids(Xd, plan, reached=True, slab_trees=slab),
                 walk.staged_margins(Xd, plan, ens.init_f, K, average),
                 walk.feature_counts(Xd, plan, F, slab_trees=slab)) for _ in range(2)]
        (ids, hit), staged, cnt = runs[0]
        assert (ids.cpu().numpy() == ids_ref).all()
        hit_ref = np.zeros((plan.T, plan.cap), np.uint8)
        hit_ref[np.arange(plan.T)[:, None], ids_ref] = 1
        assert (hit.cpu().numpy() == hit_ref).all()
        assert (staged.cpu().numpy() == want).all()
        assert (cnt.cpu().numpy() == cnt_ref).all()
        (ids2, hit2), staged2, cnt2 = runs[1]
        assert torch.equal(ids, ids2) and torch.equal(hit, hit2) and torch.equal(staged, staged2) and \
            torch.equal(cnt, cnt2)


def _model(kind: str, dev):
    from h2omx.models import (H2OGradientBoostingEstimator, H2OIsolationForestEstimator,
                              H2ORandomForestEstimator)

    rng = np.random.default_rng(7)
    n = 600
    df = pd.DataFrame(rng.normal(size=(n, 3)), columns=list("abc"))
    df.loc[::7, "c"] = np.nan
    g = rng.choice([f"L{i}" for i in range(8)], n)
    df["g"] = pd.Categorical(g)
    score = df.a - df.b + 2.0 * np.isin(g, ["L1", "L4", "L6"])
    df["y2"] = pd.Categorical(np.where(score + rng.normal(size=n) > 0.5, "p", "q"))
    df["y3"] = pd.Categorical(np.digitize(score, [-0.5, 1.5]).astype(str))
    fr = Frame.from_pandas(df, device=dev)
    x = ["a", "b", "c", "g"]
    if kind == "gbm":
        return H2OGradientBoostingEstimator(ntrees=5, max_depth=4, seed=1).train(x=x, y="y2", training_frame=fr), fr
    if kind == "multinomial":
        return H2OGradientBoostingEstimator(ntrees=4, max_depth=4, seed=1).train(x=x, y="y3", training_frame=fr), fr
    if kind == "drf":
        return H2ORandomForestEstimator(ntrees=5, max_depth=4, seed=1).train(x=x, y="y2", training_frame=fr), fr
    return H2OIsolationForestEstimator(ntrees=5, max_depth=4, seed=1).train(x=x, training_frame=fr), fr


def _same(a: Frame, b: Frame):
    assert a.names == b.names
    for c in a.names:
        va, vb = a.vec(c), b.vec(c)
        assert va.vtype == vb.vtype and va.domain == vb.domain and va.data.dtype == vb.data.dtype, c
        assert va.data.is_cuda and torch.equal(va.data, vb.data), c


@pytest.mark.parametrize("kind", ["gbm", "multinomial", "drf", "isolation"])
def test_public_methods_equal_tensor_bodies(cuda_dev, kind):
    from h2omx import explain_more as em

    m, fr = _model(kind, cuda_dev)
    X = em._X(m, fr).float()
    assert em.walk_engine(m, X) == "hip" and em.walk_engine(m, X, path=True) == "hip"
    if kind == "gbm":
        assert m.ens.catbits is not None and bool((m.ens.trees["na_left"] & 2).any())      # a group split is walked
    _same(m.predict_leaf_node_assignment(fr, "Path"), em._leaf_torch(m, X, "Path"))
    _same(m.predict_leaf_node_assignment(fr, "Node_ID"), em._leaf_torch(m, X, "Node_ID"))
    _same(m.feature_frequencies(fr), em._frequencies_torch(m, X))
    if kind != "isolation":      # an Isolation Forest has no link: staged_predict_proba raises on every route
        _same(m.staged_predict_proba(fr), em._staged_torch(m, X))


def test_refusals(cuda_dev):
    from h2omx.ops import walk

    X, trees, catbits, _, _ = _case(257, 5)
    plan = walk.pack_walk(_ens(trees, catbits, 1, True), cuda_dev)
    for call in (lambda: walk.leaf_ids(torch.from_numpy(X), plan),
                 lambda: walk.staged_margins(torch.from_numpy(X), plan, np.zeros(1), 1, True),
                 lambda: walk.feature_counts(torch.from_numpy(X), plan, 5),
                 lambda: walk.leaf_ids(torch.from_numpy(X[:3]).to(cuda_dev), plan)):     # a split feature has no row
        with pytest.raises(ValueError):
            call()
    bad = trees.copy()
    bad[1]["left"][0] = trees.shape[1] - 1          # left + 1 lies outside the tree
    with pytest.raises(ValueError):
        walk.pack_walk(_ens(bad, catbits, 1, True), cuda_dev)
    bad = trees.copy()
    bad[5]["left"][7] = 3                           # a child before its parent
    with pytest.raises(ValueError):
        walk.pack_walk(_ens(bad, catbits, 1, True), cuda_dev)
