"""Level finalisation in the consumer kernel's prologue (HipTreeBuilder.FIN_PROLOGUE):
every workgroup of the launch that routes a level's rows finalises the level
for itself and block 0 stores the results, instead of a one-workgroup
node_best_finalize launch per level.  Both paths run the same integer
histograms and the same fp64 decision code, so trees and margins must be equal
byte for byte - no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from h2omx.models.tree import TreeParams, bin_matrix, compute_edges, train_ensemble

pytestmark = pytest.mark.gpu

F = 7
N_SMALL = 2999     # a partial 16-row unit and a partial wave
N_WIDE = 70001     # with TARGET_WGS = 8 / MIN_GROUPS = 2: several workgroups in each of >= 2 feature groups


def _data(n, seed=0, task="bin"):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(F, n)).astype(np.float32)
    X[2, rng.random(n) < 0.1] = np.nan
    X[5] = rng.integers(0, 3, n)   # 3-valued column
    logit = 1.5 * X[0] - X[1] * X[3] + np.nan_to_num(X[2]) + 0.7 * X[5] + 0.5 * np.sin(3 * X[4])
    if task == "bin":
        y = (rng.random(n) < 1 / (1 + np.exp(-logit))).astype(np.float32)
    else:
        y = (logit + rng.normal(size=n)).astype(np.float32)
    return X, y


_cache = {}


def _binned(n, nbins, task, cat=False):
    """device BinnedMatrix + labels, built once per shape and left unchanged"""
    key = (n, nbins, task, cat)
    if key not in _cache:
        X, y = _data(n, seed=n % 97 + nbins, task=task)
        if cat:
            X[6] = np.random.default_rng(5).integers(0, 23, n)   # enum column, 23 levels
            y = (y + (X[6] % 3 == 0)).astype(np.float32) if task != "bin" else y
        Xt = torch.from_numpy(X)
        e, nv, nbt = compute_edges(Xt, nbins)
        cf = None
        if cat:
            from h2omx.models.tree.binning import categorical_bins

            e, nv, nbt, cf = categorical_bins(e, nv, nbt, {6: 23})
        bm = bin_matrix(Xt.cuda(), e, nv, nbt, cat=cf)
        _cache[key] = (bm, torch.from_numpy(y).cuda())
    return _cache[key]


def _reach(tr):
    keep, stack = [], [0]
    while stack:
        i = stack.pop()
        keep.append(i)
        if tr[i]["feat"] >= 0:
            stack += [int(tr[i]["left"]), int(tr[i]["left"]) + 1]
    return sorted(keep)


def _leaf_depths(tr):
    out, stack = [], [(0, 0)]
    while stack:
        i, d = stack.pop()
        if tr[i]["feat"] >= 0:
            stack += [(int(tr[i]["left"]), d + 1), (int(tr[i]["left"]) + 1, d + 1)]
        else:
            out.append(d)
    return out


def _assert_identical(a, b):
    assert a.trees.shape == b.trees.shape
    for t in range(a.trees.shape[0]):
        ra = _reach(a.trees[t])
        assert ra == _reach(b.trees[t]), t
        # every field of every reachable record (unreachable heap slots are never written)
        assert a.trees[t][ra].tobytes() == b.trees[t][ra].tobytes(), f"tree {t}"
        if a.catbits is not None:
            assert a.catbits[t][ra].tobytes() == b.catbits[t][ra].tobytes(), f"tree {t} bitsets"
    fa, fb = a._state.Fm.cpu().numpy(), b._state.Fm.cpu().numpy()
    assert fa.tobytes() == fb.tobytes()


class _Calls:
    """counts the native launches of the two paths"""

    NAMES = ("h2omx_level_finalize", "h2omx_hist_build_route_fin", "h2omx_partition_route_fin",
             "h2omx_partition_final_fin")

    def __init__(self, monkeypatch):
        from h2omx import ops

        lib = ops.tree_lib()
        self.n = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)))

    def _wrap(self, name, fn):
        def call(*a):
            self.n[name] += 1
            return fn(*a)
        return call

    def take(self):
        out, self.n = self.n, dict.fromkeys(self.NAMES, 0)
        return out


def _off_on(monkeypatch, bm, y, *, dist, tp, ntrees=3, wide=False):
    import h2omx.models.tree.engine as E

    # all three consumer sites (the default keeps the last level's launch: see test_prologue_default_sites)
    monkeypatch.setattr(E.HipTreeBuilder, "FIN_PROLOGUE_FINAL", True)
    if wide:
        monkeypatch.setattr(E.HipTreeBuilder, "TARGET_WGS", 8)   # few, large row chunks
        monkeypatch.setattr(E.HipTreeBuilder, "MIN_GROUPS", 2)   # >= 2 feature groups on every level
    calls = _Calls(monkeypatch)
    out = {}
    for flag in (False, True):
        monkeypatch.setattr(E.HipTreeBuilder, "FIN_PROLOGUE", flag)
        out[flag] = train_ensemble(bm, y, dist=dist, ntrees=ntrees, tparams=tp, seed=3)
        n = calls.take()
        if flag:   # every level of these trees (<= 32 nodes, one pass) qualifies
            assert n["h2omx_level_finalize"] == 0, n
            assert n["h2omx_partition_final_fin"] > 0, n
            if tp.max_depth >= 2:
                assert n["h2omx_hist_build_route_fin"] > 0, n
            if tp.max_depth >= 5:
                assert n["h2omx_partition_route_fin"] > 0, n
        else:
            assert n["h2omx_level_finalize"] > 0 and sum(n.values()) == n["h2omx_level_finalize"], n
    _assert_identical(out[False], out[True])
    return out[True]


# depth 2: one routed level + the final partition; 5: the headline's sequence
# (three routed histograms, one partition_route, the final partition); 6: two
# partition_route levels.  mode 0: relative min_split_improvement; mode 1: XGBoost gain
@pytest.mark.parametrize("n,depth,nbins,dist,mode", [
    (N_SMALL, 2, 255, "bernoulli", 0), (N_SMALL, 3, 31, "bernoulli", 1), (N_SMALL, 5, 255, "gaussian", 0),
    (N_SMALL, 6, 31, "bernoulli", 0), (N_WIDE, 2, 255, "bernoulli", 1), (N_WIDE, 3, 31, "gaussian", 0),
    (N_WIDE, 5, 255, "bernoulli", 0), (N_WIDE, 6, 255, "bernoulli", 1), (N_WIDE, 6, 31, "gaussian", 1)])
def test_prologue_matches_finalize_launch(cuda_dev, monkeypatch, n, depth, nbins, dist, mode):
    bm, y = _binned(n, nbins, "bin" if dist == "bernoulli" else "reg")
    tp = TreeParams(max_depth=depth, min_rows=3, learn_rate=0.2, mode=mode, reg_lambda=1.0 if mode else 0.0,
                    min_split_improvement=0.0 if mode else 1e-5)
    wide = n == N_WIDE
    if wide:
        import h2omx.models.tree.engine as E

        made = []
        init = E.HipTreeBuilder.__init__

        def spy(self, *a, **k):
            init(self, *a, **k)
            made.append(self)

        monkeypatch.setattr(E.HipTreeBuilder, "__init__", spy)
    _off_on(monkeypatch, bm, y, dist=dist, tp=tp, wide=wide)
    if wide:
        # non-writer workgroups decide real rows from their local copies: more than
        # one feature group and more than one row chunk per group on the routed levels
        for slots in (1, 2, 4):
            plan = made[-1].plan_level(slots)
            assert plan["n_groups"] >= 2 and plan["wgpg"] >= 8 and plan["passes"] == 1, plan


@pytest.mark.parametrize("n,depth,min_rows", [(N_SMALL, 6, 250.0), (N_WIDE, 5, 9000.0)])
def test_prologue_early_leaves_and_short_trees(cuda_dev, monkeypatch, n, depth, min_rows):
    """min_rows large enough that nodes refuse to split and a tree ends before
    max_depth: a level finalises with 0 children and the launches after it see
    n_prev = 0 / 0 slots (block 0 still writes the control blocks they read)."""
    bm, y = _binned(n, 255, "bin")
    tp = TreeParams(max_depth=depth, min_rows=min_rows, learn_rate=0.3, min_split_improvement=1e-5)
    ens = _off_on(monkeypatch, bm, y, dist="bernoulli", tp=tp, ntrees=4, wide=n == N_WIDE)
    ld = [_leaf_depths(t) for t in ens.trees]
    assert min(max(d) for d in ld) < depth, ld      # a tree ended before max_depth
    assert any(min(d) < max(d) for d in ld), ld     # a node refused to split while its level went on


@pytest.mark.parametrize("case", ["monotone", "interactions", "categorical", "col_sample"])
def test_prologue_side_effects(cuda_dev, monkeypatch, case):
    """The writer block's other stores: children's value intervals (gbound),
    interaction states (istate), the tree's categorical bitsets (treecat; the
    local records test the scan's copy), and per-tree feature masks upstream."""
    kw = {}
    cat = case == "categorical"
    if case == "monotone":
        kw = dict(monotone=(1, 0, 0, -1, 0, 0, 0))
    elif case == "interactions":
        kw = dict(interactions=((0, 1), (2, 3, 5)))
    elif case == "col_sample":
        kw = dict(col_sample_rate=0.6)
    dist = "gaussian" if case in ("monotone", "categorical") else "bernoulli"
    bm, y = _binned(N_WIDE if cat else N_SMALL, 255, "bin" if dist == "bernoulli" else "reg", cat=cat)
    tp = TreeParams(max_depth=5, min_rows=5, learn_rate=0.2, seed=5, **kw)
    ens = _off_on(monkeypatch, bm, y, dist=dist, tp=tp, wide=cat)
    if cat:
        assert ens.catbits is not None
        assert any(int(t[i]["na_left"]) & 2 for t in ens.trees for i in _reach(t)), "no categorical split was chosen"


def test_prologue_graph_replay(cuda_dev, monkeypatch):
    """4 trees with the prologue on: graph replay (chained steps) against the
    eager launch sequence, then both against the finalisation launch."""
    import h2omx.models.tree.engine as E
    from h2omx.models.tree import boost as B

    bm, y = _binned(N_WIDE, 255, "bin")
    tp = TreeParams(max_depth=5, min_rows=10, learn_rate=0.2)
    monkeypatch.setattr(E.HipTreeBuilder, "TARGET_WGS", 8)
    made = []
    init = B.GpuBooster.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        made.append(self)

    monkeypatch.setattr(B.GpuBooster, "__init__", spy)
    out = {}
    for pro, graph in ((True, "0"), (True, "1"), (False, "1")):
        monkeypatch.setattr(E.HipTreeBuilder, "FIN_PROLOGUE", pro)
        monkeypatch.setenv("H2OMX_TREE_GRAPH", graph)
        out[(pro, graph)] = train_ensemble(bm, y, dist="bernoulli", ntrees=4, tparams=tp, seed=5)
    assert not made[0].graph_used and made[1].graph_used and made[2].graph_used, (made[1].graph_error,
                                                                                  made[2].graph_error)
    _assert_identical(out[(True, "0")], out[(True, "1")])
    _assert_identical(out[(False, "1")], out[(True, "1")])


def test_prologue_default_sites(cuda_dev, monkeypatch):
    """Default switches: the routed histograms and partition_route finalise their
    levels, the last level keeps its one launch per tree (measured slower in
    partition_final's prologue) - same trees and margins as every launch."""
    import h2omx.models.tree.engine as E

    bm, y = _binned(N_WIDE, 255, "bin")
    tp = TreeParams(max_depth=5, min_rows=10, learn_rate=0.2)
    monkeypatch.setattr(E.HipTreeBuilder, "TARGET_WGS", 8)
    monkeypatch.setattr(E.HipTreeBuilder, "MIN_GROUPS", 2)
    monkeypatch.setenv("H2OMX_TREE_GRAPH", "0")   # every tree's launches go through the counted entry points
    assert E.HipTreeBuilder.FIN_PROLOGUE and not E.HipTreeBuilder.FIN_PROLOGUE_FINAL
    calls = _Calls(monkeypatch)
    on = train_ensemble(bm, y, dist="bernoulli", ntrees=3, tparams=tp, seed=3)
    n = calls.take()
    assert n == {"h2omx_level_finalize": 3, "h2omx_hist_build_route_fin": 9, "h2omx_partition_route_fin": 3,
                 "h2omx_partition_final_fin": 0}, n
    monkeypatch.setattr(E.HipTreeBuilder, "FIN_PROLOGUE", False)
    off = train_ensemble(bm, y, dist="bernoulli", ntrees=3, tparams=tp, seed=3)
    assert calls.take()["h2omx_level_finalize"] == 15
    _assert_identical(off, on)
