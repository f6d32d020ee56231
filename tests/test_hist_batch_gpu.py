"""hist_build's batched loop (HipTreeBuilder.HIST_BATCH): level 0 loads a row
unit's packed rows and the codes of all the group's planes together, consumes
them in issue order and adds every row unmasked (rows outside the histogram
add 0).  The plain last level measured slower with that loop
(profiles/r14/hist_stream_ab.txt): the engine keeps the feature loop there,
which the depth-5 cases pin.  The sums are the same int64
values, so every tree and margin must be bit-identical

* to the exact fixed-point oracle (tests/quantref.py), node by node, as in
  tests/test_tree_oracle_gpu.py (eager fits: a spy records each tree), and
* to the same build with ``HIST_BATCH = False`` (the feature loop).

Rows: 1, 15, 17, 1023 (a partial row unit / workgroup step), 16385 and
3 * 16384 + 5 (more than one workgroup step, padding rows in the last unit).
Features: 1 (nf = 1), 2, 7 (nf < FG_MAX), 8, 9 (a short last group), 28 (four
groups; three 3-valued columns that BUNDLE joins into one plane).  Column 0
holds NA codes.  Depth 1 is level 0 alone; depth 5 adds the routed levels and
the plain last one, which read the rows level 0 stored.  A spy on ``h2omx_hist_build`` pins which loop
each launch asked for (mode bit 7) and the group width it was given.  The
planner spreads shards this small over one-plane groups (SMALL_SHARD), so the
cases that are about the group width switch that off, as the planner tests do;
test_default_planner keeps it.

The 16-bit packed rows (PK32: level 0 is PKM 3) need >= 65536 rows per
workgroup, and the level-0 kernel that reads the rows boost_update packed
(PKM 6, chained graph replay) needs PK32: those cases run 600005 rows on 8 workgroups per group."""
import copy

import numpy as np
import pytest
import torch

import quantref as Q
from h2omx.models.tree import TreeParams, bin_matrix, compute_edges, train_ensemble
from h2omx.models.tree.engine import trees_from_bytes

pytestmark = pytest.mark.gpu

SEED = 3
ROWS = [1, 15, 17, 1023, 16385, 3 * 16384 + 5]
FEATS = [1, 2, 7, 8, 9, 28]
N_PK32 = 600_005
_cache = {}


def _data(n, F):
    """(X [F][n], y, edges, nvb, nbt, host codes), computed once and left unchanged: normal columns, 10 % NaN
    in column 0, the last three of >= 7 columns 3-valued (bundled into one joint plane)"""
    if (n, F) not in _cache:
        rng = np.random.default_rng(1000 * F + n % 997)
        X = rng.normal(size=(F, n)).astype(np.float32)
        X[0, rng.random(n) < 0.1] = np.nan
        if F >= 7:
            X[F - 3:] = rng.integers(0, 3, (3, n))
        logit = 1.2 * np.nan_to_num(X[0]) - X[F // 2] + 0.8 * X[F - 1]
        y = (rng.random(n) < 1 / (1 + np.exp(-logit))).astype(np.float32)
        Xt = torch.from_numpy(X)
        e, nv, nbt = compute_edges(Xt, 255)
        codes = bin_matrix(Xt, e, nv, nbt).codes.numpy()[:, :n].copy()
        for a in (X, y, e, nv, codes):
            a.setflags(write=False)
        _cache[(n, F)] = (X, y, e, nv, nbt, codes)
    return _cache[(n, F)]


def _fit(monkeypatch, n, F, batch, *, depth=5, ntrees=2, mode=0, graph="0", attrs=None, spy_trees=False):
    """(ensemble, binned matrix, recorded trees, recorded h2omx_hist_build launches (pkm, F, fg, slot_cnt))"""
    import h2omx.models.tree.engine as E
    from h2omx import ops

    monkeypatch.setenv("H2OMX_TREE_GRAPH", graph)
    monkeypatch.setenv("H2OMX_TREE_ENGINE", "scan")
    monkeypatch.setattr(E.HipTreeBuilder, "HIST_BATCH", batch)
    for k, v in (attrs or {}).items():
        monkeypatch.setattr(E.HipTreeBuilder, k, v)
    X, y, e, nv, nbt, _ = _data(n, F)
    bm = bin_matrix(torch.tensor(X).cuda(), e.copy(), nv.copy(), nbt)
    calls, launches = [], []
    build = E.HipTreeBuilder.build

    def spy(self, g, h, w, tree_index, tree_fmask=None, grad_fuse=None, stat=None, chain=False):
        rec = dict(builder=self, tree_index=tree_index, p=copy.copy(self.p), g=g[:n].clone(), h=h[:n].clone(),
                   w=None if w is None else w[:n].clone(), fmask=None if tree_fmask is None else tree_fmask.clone(),
                   stat=(self.stat_max if stat is None else stat).clone())
        out = build(self, g, h, w, tree_index, tree_fmask, grad_fuse, stat, chain)
        rec.update(tree=out.clone(), qscale=self.qscale.clone(), nid=self.nid[:n].clone(), pk=self.pk.clone())
        calls.append(rec)
        return out

    if spy_trees:
        monkeypatch.setattr(E.HipTreeBuilder, "build", spy)
    lib = ops.tree_lib()
    hist_build = lib.h2omx_hist_build

    def spy_hist(*a):
        launches.append(dict(pkm=a[21], F=a[10], fg=a[12], slot_cnt=a[16]))
        return hist_build(*a)

    monkeypatch.setattr(lib, "h2omx_hist_build", spy_hist)
    if mode == 0:
        tp = TreeParams(seed=5, max_depth=depth, min_rows=1.0, learn_rate=0.3)
    else:   # XGBoost mode: s2 = h
        tp = TreeParams(seed=5, max_depth=depth, mode=1, reg_lambda=1.0, min_child_weight=1.0, gamma=0.0, learn_rate=0.3)
    ens = train_ensemble(bm, torch.tensor(y).cuda(), dist="bernoulli", ntrees=ntrees, tparams=tp, seed=SEED)
    torch.cuda.synchronize()
    monkeypatch.setattr(lib, "h2omx_hist_build", hist_build)
    if spy_trees:
        monkeypatch.setattr(E.HipTreeBuilder, "build", build)
    return ens, bm, calls, launches


def _np(t):
    return None if t is None else t.cpu().numpy()


def _oracle(n, F, ens, bm, calls):
    """every recorded tree against quantref, then the margins bit for bit"""
    _, _, e, nv, nbt, codes = _data(n, F)
    assert np.array_equal(bm.codes.cpu().numpy()[:, :n], codes)
    margin = np.repeat(ens.init_f.astype(np.float32)[:, None], n, 1)
    ties = []
    for j, r in enumerate(calls):
        b, p, ti = r["builder"], r["p"], r["tree_index"]
        want = Q.scales(_np(r["stat"]), p.mode, b.max_rows_per_wg)
        g, h, w = _np(r["g"]), _np(r["h"]), _np(r["w"])
        nid = _np(r["nid"])
        tree = trees_from_bytes(_np(r["tree"]), b.capacity)[0]
        ties.append(Q.verify(codes, nv, e, g, h, w, p, want, b.row_base, ti & 0x7FFFFFFF, _np(r["fmask"]), tree, nid,
                             _np(r["qscale"]), tree_index=ti))
        gq, sq = Q.quantised_rows(g, h, w, p.mode, want, b.row_base, ti & 0x7FFFFFFF)
        pk = r["pk"].view(torch.int32)[:n] if b.pk32 else r["pk"][:n]
        got = _np(pk).view(np.uint32 if b.pk32 else np.uint64)
        assert np.array_equal(got, Q.packed_rows(gq, sq, b.pk32)), f"tree {j}: packed rows"
        margin[0] += tree["value"][~nid.astype(np.int64)]
    assert len(calls) == ens.trees.shape[0]
    assert ens._state.Fm[:, :n].cpu().numpy().tobytes() == margin.tobytes(), "training margins"
    assert max(ties) <= 1, ties


def _same(a, b):
    assert a.trees.shape == b.trees.shape
    for t in range(a.trees.shape[0]):
        reach = a.compact()[t]
        assert reach == b.compact()[t], t
        for f in ("feat", "bin", "na_left", "value", "weight"):
            np.testing.assert_array_equal(a.trees[t][reach][f], b.trees[t][reach][f], err_msg=f"tree {t} {f}")
    assert torch.equal(a._state.Fm, b._state.Fm)


def _l0(launches):
    return [c for c in launches if (c["pkm"] & 7) in (1, 3, 6)]


def _batched(launches):
    return [c for c in launches if c["pkm"] & 128]


WIDE = dict(SMALL_SHARD=False, BUNDLE=False)   # groups as wide as the LDS budget allows, one plane per feature


@pytest.mark.parametrize("depth", [1, 5])
@pytest.mark.parametrize("F", FEATS)
@pytest.mark.parametrize("n", ROWS)
def test_batched_loop_matches_oracle_and_feature_loop(cuda_dev, monkeypatch, n, F, depth):
    on, bm, calls, launches = _fit(monkeypatch, n, F, True, depth=depth, attrs=WIDE, spy_trees=True)
    _oracle(n, F, on, bm, calls)
    # level 0 of every tree asked for the batched loop, in equal groups of <= 8
    # planes (8 lane copies: 8 planes fill the LDS budget): 1, 2, 7, 8, 5 + 4 and
    # 4 x 7; the plain last level of a depth-5 tree (stored rows: PKM 2) did not
    fg0 = -(-F // -(-F // 8))
    l0 = [c for c in launches if (c["pkm"] & 7) in (1, 3, 6)]
    assert len(l0) >= 2 and all(c["pkm"] & 128 and c["fg"] == fg0 and c["slot_cnt"] == 1 for c in l0), launches
    deep = [c for c in launches if (c["pkm"] & 7) in (2, 4)]
    # (the engine keeps the feature loop there: it measured slower with the batched one)
    assert all(not c["pkm"] & 128 and c["slot_cnt"] == 8 for c in deep), launches
    assert bool(deep) == (depth == 5), launches
    off, _, _, launches_off = _fit(monkeypatch, n, F, False, depth=depth, attrs=WIDE)
    assert not _batched(launches_off)
    _same(on, off)


@pytest.mark.parametrize("cop", [1, 4, 8])
@pytest.mark.parametrize("bundle", [True, False])
def test_level0_copies_and_bundled_planes(cuda_dev, monkeypatch, cop, bundle):
    """L0_COPIES 1 / 4 / 8 (plain slices - the 3-valued columns replicated inside theirs - or interleaved lane
    copies), with the 3-valued columns bundled into a joint plane or one plane each"""
    n, F = ROWS[-1], 28
    attrs = dict(L0_COPIES=cop, BUNDLE=bundle, SMALL_SHARD=False)
    on, bm, calls, launches = _fit(monkeypatch, n, F, True, attrs=attrs, spy_trees=True)
    assert (calls[0]["builder"].planes is not None) == bundle
    _oracle(n, F, on, bm, calls)
    planes = {c["F"] for c in launches}
    assert len(planes) == 1 and (max(planes) < 28 if bundle else planes == {28}), planes
    assert all(c["pkm"] & 128 and 5 <= c["fg"] <= 8 for c in _l0(launches)), launches
    off, _, _, _ = _fit(monkeypatch, n, F, False, attrs=attrs)
    _same(on, off)


@pytest.mark.parametrize("n", [17, ROWS[-1]])
def test_default_planner(cuda_dev, monkeypatch, n):
    """every switch at its default: shards this small run one-plane groups (nf = 1)"""
    F = 28
    on, bm, calls, launches = _fit(monkeypatch, n, F, True, spy_trees=True)
    assert _l0(launches) and all(c["pkm"] & 128 for c in _l0(launches)), launches
    _oracle(n, F, on, bm, calls)
    off, _, _, _ = _fit(monkeypatch, n, F, False)
    _same(on, off)


def test_group_wider_than_fg_max_keeps_the_feature_loop(cuda_dev, monkeypatch):
    """without the planner's cap a 28-plane group reaches the launcher with the mode bit set: it runs the feature loop"""
    n, F = ROWS[-1], 28
    attrs = dict(L0_COPIES=1, BUNDLE=False, SMALL_SHARD=False, HIST_FG_MAX=64)
    on, bm, calls, launches = _fit(monkeypatch, n, F, True, attrs=attrs, spy_trees=True)
    assert any(c["pkm"] & 128 and c["fg"] == 28 for c in launches), launches
    _oracle(n, F, on, bm, calls)
    off, _, _, _ = _fit(monkeypatch, n, F, False, attrs=attrs)
    _same(on, off)


def test_xgboost_mode(cuda_dev, monkeypatch):
    """second-order gain: the histograms' second plane is h (s2 = h)"""
    n, F = ROWS[-1], 9
    on, bm, calls, launches = _fit(monkeypatch, n, F, True, mode=1, attrs=WIDE, spy_trees=True)
    assert calls[0]["p"].mode == 1 and all(c["pkm"] & 128 and c["fg"] > 1 for c in _l0(launches)), launches
    _oracle(n, F, on, bm, calls)
    off, _, _, _ = _fit(monkeypatch, n, F, False, mode=1, attrs=WIDE)
    _same(on, off)


@pytest.mark.parametrize("pk32", [True, False])
def test_packed_rows_16_and_64_bit(cuda_dev, monkeypatch, pk32):
    """level 0 storing 16-bit rows (PK32: PKM 3) or 64-bit rows (PKM 1) in the batched loop, at the size where
    PK32 applies; the plain last level reads them back in the feature loop (PKM 4 / 2)"""
    n, F = N_PK32, 9
    attrs = dict(TARGET_WGS=8, PK32=pk32)
    on, bm, calls, launches = _fit(monkeypatch, n, F, True, attrs=attrs, spy_trees=True)
    assert calls[0]["builder"].pk32 == pk32
    assert {c["pkm"] & 7 for c in launches} == ({3, 4} if pk32 else {1, 2}), launches
    assert all(c["pkm"] & 128 for c in _l0(launches))
    _oracle(n, F, on, bm, calls)
    off, _, _, _ = _fit(monkeypatch, n, F, False, attrs=attrs)
    _same(on, off)


def test_chained_graph_replay_of_four_trees(cuda_dev, monkeypatch):
    """graph replay: level 0 of the chained trees reads the rows boost_update packed (PKM 6); the replayed
    trees equal the eager ones (held to the oracle above) and the feature loop's"""
    n, F = N_PK32, 9
    attrs = dict(TARGET_WGS=8)
    on, _, _, launches = _fit(monkeypatch, n, F, True, ntrees=4, graph="1", attrs=attrs)
    assert any((c["pkm"] & 7) == 6 and c["pkm"] & 128 for c in launches), launches
    eager, bm, calls, _ = _fit(monkeypatch, n, F, True, ntrees=4, attrs=attrs, spy_trees=True)
    _oracle(n, F, eager, bm, calls)
    _same(on, eager)
    off, _, _, launches_off = _fit(monkeypatch, n, F, False, ntrees=4, graph="1", attrs=attrs)
    assert not _batched(launches_off)
    _same(on, off)
