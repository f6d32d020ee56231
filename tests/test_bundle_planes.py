"""Joint histogram planes for low-cardinality features (HipTreeBuilder.BUNDLE,
binning.BundlePlan): features whose radices (valid bins + 1 for NA) multiply to
at most the histogram width share ONE code plane; reduce_split sums the joint
row over the other digits to get each feature's own row.  The sums are exact
int64 and the per-row quantised values do not depend on the plane, so BUNDLE on
and off must build the same trees and margins byte for byte - no tolerance
anywhere in this file."""
import numpy as np
import pytest
import torch

from h2omx.models.tree import TreeParams, bin_matrix, compute_edges, train_ensemble
from h2omx.models.tree.binning import plan_bundles

N = 20037   # not a multiple of 16 / 64 / 1024


def _labels(rng, logit):
    return (rng.random(logit.size) < 1 / (1 + np.exp(-logit))).astype(np.float32)


def _data_fill256():
    """two continuous, four 3-valued (NaNs in one), one 5-valued: the 3-valued
    columns fill a bundle to exactly 256, the 5-valued one is left over"""
    rng = np.random.default_rng(11)
    X = rng.normal(size=(7, N)).astype(np.float32)
    for f in (2, 3, 4, 5):
        X[f] = rng.integers(0, 3, N)
    X[3, rng.random(N) < 0.15] = np.nan
    X[6] = rng.integers(0, 5, N)
    logit = (0.8 * X[0] - 0.5 * X[1] + 2.0 * (X[2] == 2) - 1.5 * (X[4] == 0) + 1.0 * np.isnan(X[3])
             + 0.6 * np.nan_to_num(X[3]) - 0.8 * (X[5] == 1) + 0.3 * X[6] - 0.5)
    return X, _labels(rng, logit), 255, [[2, 3, 4, 5]]


def _data_nbt64():
    """nbins 63 (histogram width 64): three 3-valued columns, product exactly 64"""
    rng = np.random.default_rng(12)
    X = rng.normal(size=(4, N)).astype(np.float32)
    for f in (1, 2, 3):
        X[f] = rng.integers(0, 3, N)
    logit = 0.7 * X[0] + 1.8 * (X[1] == 0) - 1.4 * (X[2] == 2) + 0.9 * X[3] - 1.0
    return X, _labels(rng, logit), 63, [[1, 2, 3]]


def _data_mixed240():
    """radices 4 x 6 x 10 = 240: a stride that is no power of two, unused joint codes"""
    rng = np.random.default_rng(13)
    X = rng.normal(size=(4, N)).astype(np.float32)
    X[1] = rng.integers(0, 3, N)
    X[2] = rng.integers(0, 5, N)
    X[3] = rng.integers(0, 9, N)
    X[2, rng.random(N) < 0.1] = np.nan
    logit = 0.6 * X[0] + 1.5 * (X[1] == 1) + 0.5 * np.nan_to_num(X[2], nan=-2.0) - 0.35 * X[3] + 0.2
    return X, _labels(rng, logit), 255, [[1, 2, 3]]


DATA = {"fill256": _data_fill256, "nbt64": _data_nbt64, "mixed240": _data_mixed240}
_cache = {}


def _case(name):
    """(X, y, edges, nvb, nbt, expected bundles), computed once and left unchanged"""
    if name not in _cache:
        X, y, nbins, want = DATA[name]()
        e, nv, nbt = compute_edges(torch.from_numpy(X), nbins)
        _cache[name] = (X, y, e, nv, nbt, want)
    return _cache[name]


def _reach(tr):
    keep, stack = [], [0]
    while stack:
        i = stack.pop()
        keep.append(i)
        if tr[i]["feat"] >= 0:
            stack += [int(tr[i]["left"]), int(tr[i]["left"]) + 1]
    return sorted(keep)


def _split_feats(ens):
    return {int(tr[i]["feat"]) for tr in ens.trees for i in _reach(tr) if tr[i]["feat"] >= 0}


# ---- CPU ------------------------------------------------------------------

def test_plan_rule_and_determinism():
    nvb = [255, 254, 3, 255, 3, 5, 3, 3, 200, 9]
    a, b = plan_bundles(nvb, 256), plan_bundles(np.asarray(nvb, np.int32), 256)
    # first fit in (radix, feature) order: 4^4 = 256 is full, then 6 x 10 = 60
    assert a.bundles == [[(2, 3, 1), (4, 3, 4), (6, 3, 16), (7, 3, 64)], [(5, 5, 1), (9, 9, 6)]]
    assert a.bundles == b.bundles
    for k in ("plane_src", "plane_nvb", "feat_plane"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes()
    # planes keep feature order, a joint plane where its lowest member stood
    assert a.plane_src.tolist() == [0, 1, -1, 3, -2, 8] and a.P == 6
    assert a.plane_nvb.tolist() == [255, 254, 255, 255, 255, 200]
    assert a.feat_plane[[0, 2, 7, 9]].tolist() == [[0, 0, 0], [2, 1, 4], [2, 64, 4], [4, 6, 10]]
    # a lone candidate stays as it is; radix > nbt / 2 is no candidate; nothing to do -> None
    assert plan_bundles([255, 3], 256) is None and plan_bundles([127, 1, 255], 256).P == 2
    assert plan_bundles([128, 128], 256) is None
    lone = plan_bundles([3, 3, 3, 3, 5, 255], 256)
    assert lone.bundles == [[(0, 3, 1), (1, 3, 4), (2, 3, 16), (3, 3, 64)]] and lone.feat_plane[4].tolist() == [1, 0, 0]


@pytest.mark.parametrize("name", list(DATA))
def test_case_plans(name):
    X, y, e, nv, nbt, want = _case(name)
    plan = plan_bundles(nv, nbt)
    assert [[f for f, _, _ in m] for m in plan.bundles] == want
    prod = int(np.prod([nvk + 1 for _, nvk, _ in plan.bundles[0]]))
    assert prod == {"fill256": 256, "nbt64": 64, "mixed240": 240}[name] and prod <= nbt
    assert plan.P == X.shape[0] - len(want[0]) + 1


@pytest.mark.parametrize("name", list(DATA))
def test_joint_bincount_marginals(name):
    """encode -> joint bincount -> marginalise == per-column bincount, int64 weights, with NA"""
    X, y, e, nv, nbt, want = _case(name)
    codes = bin_matrix(torch.from_numpy(X), e, nv, nbt).codes.numpy()[:, :N]
    plan = plan_bundles(nv, nbt)
    joint = plan.encode(codes)
    assert joint.dtype == np.uint8 and joint.shape == (1, N)
    rng = np.random.default_rng(1)
    wts = rng.integers(-2 ** 40, 2 ** 40, N, dtype=np.int64)
    jh = np.zeros(nbt, np.int64)
    np.add.at(jh, joint[0], wts)
    na_seen = False
    for f in want[0]:
        own = np.zeros(nbt, np.int64)
        np.add.at(own, codes[f], wts)
        assert plan.marginal(jh, f).tobytes() == own.tobytes(), f
        na_seen |= bool(own[nbt - 1] != 0)
    assert na_seen == (name != "nbt64")


def test_builder_without_plane_count_plans_on_features():
    from h2omx.models.tree.engine import HipTreeBuilder

    def builder(**kw):
        b = HipTreeBuilder.__new__(HipTreeBuilder)
        b.F, b.nbt, b.max_rows_per_wg = 28, 256, None

        class BM:
            npad = 11_000_000 // 64 * 64
        b.bm = BM
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    bare, same, fewer = builder(), builder(n_planes=28), builder(n_planes=25)
    for s in (1, 2, 4, 8, 16, 64):
        assert bare._choose(s) == same._choose(s)
        p = fewer._choose(s)
        assert p["fg"] * p["n_groups"] >= 25 and p["fg"] * (p["n_groups"] - 1) < 25
    assert bare._choose(1)["fg"] == 28 and fewer._choose(1)["fg"] == 25


@pytest.mark.parametrize("name", list(DATA))
def test_cpu_reference_splits_on_bundled_feature(name):
    """the labels depend on the bundled columns strongly enough that the CPU
    reference builder splits on one too"""
    X, y, e, nv, nbt, want = _case(name)
    bm = bin_matrix(torch.from_numpy(X), e, nv, nbt)
    ens = train_ensemble(bm, y, dist="bernoulli", ntrees=1, tparams=TreeParams(max_depth=4, min_rows=5), seed=3)
    assert _split_feats(ens) & set(want[0])


# ---- GPU ------------------------------------------------------------------

def _assert_identical(a, b):
    assert a.trees.shape == b.trees.shape
    for t in range(a.trees.shape[0]):
        ra = _reach(a.trees[t])
        assert ra == _reach(b.trees[t]), t
        # every field of every reachable record (unreachable heap slots are never written)
        assert a.trees[t][ra].tobytes() == b.trees[t][ra].tobytes(), f"tree {t}"
    fa, fb = a._state.Fm.cpu().numpy(), b._state.Fm.cpu().numpy()
    assert fa.tobytes() == fb.tobytes()


_gpu = {}


def _binned_gpu(name):
    if name not in _gpu:
        X, y, e, nv, nbt, want = _case(name)
        _gpu[name] = (bin_matrix(torch.from_numpy(X).cuda(), e, nv, nbt), torch.from_numpy(y).cuda())
    return _gpu[name]


def _nonnull(p) -> bool:
    return p is not None and getattr(p, "value", p) not in (None, 0)


def _off_on(monkeypatch, name, mode, depth):
    import h2omx.models.tree.engine as E
    from h2omx import ops

    bm, y = _binned_gpu(name)
    X, _, e, nv, nbt, want = _case(name)
    # the device planes are what the NumPy rule says
    plan = bm.bundle
    assert plan is not None and [[f for f, _, _ in m] for m in plan.bundles] == want
    codes = bm.codes.cpu().numpy()
    assert plan.joint.cpu().numpy()[:, :N].tobytes() == plan.encode(codes[:, :N]).tobytes()
    assert not plan.joint.cpu().numpy()[:, N:].any()

    lib = ops.tree_lib()
    seen = {"planes": set(), "tables": 0, "passes": set()}
    rs = lib.h2omx_reduce_split
    hb = {k: getattr(lib, k) for k in ("h2omx_hist_build", "h2omx_hist_build_route", "h2omx_hist_build_route_fin")}

    def spy_rs(*a):
        seen["tables"] += _nonnull(a[-2])
        seen["passes"].add(a[3])      # slot_lo
        return rs(*a)

    def spy_hb(k, planes_at):
        def call(*a):
            seen["planes"].add((a[planes_at], _nonnull(a[-2])))
            return hb[k](*a)
        return call

    monkeypatch.setattr(lib, "h2omx_reduce_split", spy_rs)
    monkeypatch.setattr(lib, "h2omx_hist_build", spy_hb("h2omx_hist_build", 10))
    monkeypatch.setattr(lib, "h2omx_hist_build_route", spy_hb("h2omx_hist_build_route", 10))
    monkeypatch.setattr(lib, "h2omx_hist_build_route_fin", spy_hb("h2omx_hist_build_route_fin", 9))
    tp = TreeParams(max_depth=depth, min_rows=5, learn_rate=0.3, mode=mode, reg_lambda=1.0 if mode else 0.0)
    out = {}
    for flag in (False, True):
        monkeypatch.setattr(E.HipTreeBuilder, "BUNDLE", flag)
        seen.update(planes=set(), tables=0, passes=set())
        out[flag] = train_ensemble(bm, y, dist="bernoulli", ntrees=3, tparams=tp, seed=3)
        F = bm.F
        if flag:
            assert seen["planes"] == {(plan.P, True)} and seen["tables"] > 0, seen
        else:
            assert seen["planes"] == {(F, False)} and seen["tables"] == 0, seen
        passes = set(seen["passes"])
    _assert_identical(out[False], out[True])
    assert _split_feats(out[True]) & set(want[0]), "no split on a bundled feature"
    return passes


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["gbm", "xgb"])
@pytest.mark.parametrize("name", list(DATA))
def test_bundle_on_off_identical(monkeypatch, name, mode):
    _off_on(monkeypatch, name, mode, depth=5)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["gbm", "xgb"])
def test_bundle_on_off_identical_multipass(monkeypatch, mode):
    """depth 8: the last level has 64 build slots.  With one 64 KB histogram
    window per workgroup (the deep 128 KB window switched off, as on levels of
    fewer than DEEP_MIN_GROUPS groups) that level takes two slot passes."""
    import h2omx.models.tree.engine as E

    monkeypatch.setattr(E.HipTreeBuilder, "DEEP_LDS_BUDGET", E.HipTreeBuilder.LDS_BUDGET)
    passes = _off_on(monkeypatch, "fill256", mode, depth=8)
    assert len(passes) > 1, passes
