"""GPU-built trees against the exact fixed-point oracle (tests/quantref.py),
node by node.

Every other tree test compares one GPU path with another, or the GPU with the
float64 reference within a loose allowance.  Here a spy around
``HipTreeBuilder.build`` records each tree's inputs ((g, h, w), tree index,
column mask, gradient maxima or bounds) and outputs (tree, qscale, node ids,
packed rows) while ``train_ensemble`` runs as in production; the oracle then
recomputes every node from the rows the GPU tree routes to it and demands
equality: scales, packed rows, split feature / bin / NA direction / child
numbering / threshold, gain and weight (1 ulp of fp32), leaf values and
weights from the fixed-point leaf sums (1 ulp), the leaf of every row, and the
training margins bit for bit.  Near-tie nodes per tree on the MI355X: 0 in
every case (at most 1 is allowed).

The (g, h, w) a tree starts from are pinned as well (tests/gradref.py): they
are the reference gradients of the margins reconstructed so far - bit for bit
for gaussian, laplace, quantile, huber and drf, within the fp32 bound of the
exp for the others - w is observation weight x bag weight exactly, and the
maxima the scales come from are those of the recorded arrays, or the fixed
bounds, which the arrays then do not exceed.  So an eager GPU fit is pinned
from the data to the margins.  Worst err / tol of the recorded gradients on the
MI355X: bernoulli 0.105 (scan_defaults 0.096, xgb 0.105, two_slot_passes
0.096, pk32 0.094), multinomial 0.067, poisson_w 0.122, gamma 0.119, tweedie
0.141; the exact class matches bit for bit.  Near-tie nodes per tree of
poisson_w, gamma, tweedie, laplace, quantile_bag and huber_w: 0 in all 18.

Categorical set splits, monotone and interaction constraints are held to the
same oracle: eight more cases (cat_gauss, cat_bern_256, cat_seg_drf,
mono_sqerr, mono_newton, mono_xgb, inter_scan, inter_seg_deep), the left-set
bitsets word for word (the builder's and the ensemble's copy), internal node
values within 1 ulp, and split_find's categorical instantiation on histograms
of the test's own.  Scoring closes the chain for every case, old and new:
raw_margin on the raw training data and predict_binned on the device codes
give the reconstructed margins bit for bit (DRF after the same in-place
division).  Near-tie nodes per tree on the MI355X: cat_gauss [0, 0, 0],
cat_bern_256 [0, 0], cat_seg_drf [0, 0], mono_sqerr [0, 0, 0], mono_newton
[0, 0, 0], mono_xgb [0, 0, 0], inter_scan [0, 0, 0], inter_seg_deep [0, 0];
worst gradient err / tol 0.085 (the two bernoulli cases).  No tolerance was
added: the mono_newton re-derivation holds the oracle's 1 ulp of fp32 as well.

Measured on the MI355X: the 20 new GPU tests (8 cases, 12 synthetic scans)
take under 2 s together, none over 0.4 s; this module's 41 tests 5.0 s; the
whole suite 419 s (784 passed, 5 skipped, none of them in the oracle modules).  The parent
commit's total was not measured beside it: it is this run less the new tests
(these 20 and 42 CPU tests of about 3 s).

Sensitivity, each edit on a throwaway build of csrc/tree_kernels.hip (new test
that fails and the field it names; the older GPU tests of the three features,
test_categorical_splits / test_monotone / test_interaction, beside it):
* ``j <= bin`` -> ``j < bin`` in feat_best_cat_wave's all-pairs pass: the three
  categorical cases at "feat/bin/na_left" (level 0) and all 12 synthetic scans
  (FeatBest "code"); old: test_categorical_gpu_matches_reference fails, 2 of 2.
* ``bin <= wb`` -> ``bin < wb`` in the left set: the three cases at "bitset"
  (one word off by the winner's bit), all 12 synthetic scans at "fbcat"; old:
  the same 2 fail.
* mono_ok's comparison flipped: the three monotone cases at "feat/bin/na_left"
  (level 0); old: 3 tests of test_monotone fail.
* ``lhi = mid; rlo = mid`` swapped with the other branch in lf_write_node: the
  three monotone cases at "value" of gid 1; old: 1 of test_monotone's 3 fails.
* the same swap in mono_newton_kernel: mono_sqerr and mono_newton at a leaf's
  "value" (mono_xgb does not run that kernel and passes); old: 2 of 3 fail.
* the right child's ``c_mask`` written as 0 in inter_children: both
  interaction cases at "feat" of gid 2 (a leaf where the oracle splits); old:
  green, test_interaction passes.
* ``b > 255`` -> ``b > 254`` in cat_left: the off-domain frame of cat_gauss and
  cat_bern_256 (raw_margin of the rows holding 255 and 255.999 under an
  NA-left split); old: green."""
import copy
import math

import numpy as np
import pytest
import torch

import gradref as GR
import quantref as Q
from oracle_cases import CASES, NEW_CASES, case_catf, case_data, case_weights, case_witnesses, tree_params
from h2omx.models.tree import bin_matrix, train_ensemble
from h2omx.models.tree.engine import GRAD_BOUNDS, trees_from_bytes
from treecmp import reachable

SEED = 3      # train_ensemble's seed in every case (the bag hash)

pytestmark = pytest.mark.gpu


def _train_spied(monkeypatch, name):
    """(ensemble, binned matrix, one record per built tree) of a case"""
    import h2omx.models.tree.engine as E
    from h2omx import ops

    c = CASES[name]
    monkeypatch.setenv("H2OMX_TREE_GRAPH", "0")
    monkeypatch.setenv("H2OMX_TREE_ENGINE", c["engine"])
    for k, v in c["attrs"].items():
        monkeypatch.setattr(E.HipTreeBuilder, k, v)
    assert not E.HipTreeBuilder.FUSE_GRAD
    X, y, e, nv, nbt, host_codes = case_data(name)
    catf = case_catf(name)
    bm = bin_matrix(torch.tensor(X).cuda(), e.copy(), nv.copy(), nbt, cat=None if catf is None else catf.copy())
    calls, direct_modes, newton = [], [], []
    build = E.HipTreeBuilder.build

    def spy(self, g, h, w, tree_index, tree_fmask=None, grad_fuse=None, stat=None, chain=False):
        assert grad_fuse is None and not chain
        n = self.bm.n
        rec = dict(builder=self, tree_index=tree_index, p=copy.copy(self.p), g=g[:n].clone(), h=h[:n].clone(),
                   w=None if w is None else w[:n].clone(),
                   fmask=None if tree_fmask is None else tree_fmask.clone(),
                   stat=(self.stat_max if stat is None else stat).clone(), fixed=stat is not None)
        before = len(newton)
        out = build(self, g, h, w, tree_index, tree_fmask, grad_fuse, stat, chain)
        rec.update(tree=out.clone(), qscale=self.qscale.clone(), nid=self.nid[:n].clone(), pk=self.pk.clone(),
                   cat=None if self.treecat is None else self.treecat.clone(), newton=len(newton) - before)
        calls.append(rec)
        return out

    monkeypatch.setattr(E.HipTreeBuilder, "build", spy)
    lib = ops.tree_lib()
    seg_direct, finalize_mono = lib.h2omx_seg_direct, lib.h2omx_leaf_finalize_mono

    def spy_direct(*a):
        direct_modes.append(a[15])     # dmode: 0 workgroup per node, 1 wave per node, 2 workgroup per row chunk
        return seg_direct(*a)

    def spy_mono(*a):
        newton.append(1)               # leaf_finalize + mono_newton_kernel instead of the plain leaf finalisation
        return finalize_mono(*a)

    monkeypatch.setattr(lib, "h2omx_seg_direct", spy_direct)
    monkeypatch.setattr(lib, "h2omx_leaf_finalize_mono", spy_mono)
    wobs = case_weights(name)
    ens = train_ensemble(bm, torch.tensor(y).cuda(), w=None if wobs is None else torch.tensor(wobs).cuda(),
                         dist=c["dist"], ntrees=c["ntrees"], tparams=tree_params(name),
                         sample_rate=c.get("sample_rate", 1.0), nclass=c.get("nclass", 1), seed=SEED,
                         dist_kw=c.get("dist_kw"))
    torch.cuda.synchronize()
    assert np.array_equal(bm.codes.cpu().numpy()[:, : bm.n], host_codes)
    return ens, bm, calls, direct_modes


def _np(t):
    return None if t is None else t.cpu().numpy()


def _verify_all(name, ens, bm, calls):
    """assertions a - j on every recorded tree; near-tie nodes per tree"""
    c = CASES[name]
    X, y, e, nv, nbt, codes = case_data(name)
    n, K = bm.n, ens.K
    assert len(calls) == c["ntrees"] * K
    wobs, rate, dist = case_weights(name), c.get("sample_rate", 1.0), c["dist"]
    catf = case_catf(name)
    ties, ratio, infos = [], 0.0, []
    margin = np.repeat(ens.init_f.astype(np.float32)[:, None], n, 1)
    for j, r in enumerate(calls):
        b, p, ti = r["builder"], r["p"], r["tree_index"]
        assert ti == j
        # i. the gradients are those of the margins so far (multinomial: at the
        # start of the iteration, every class), the weights observation x bag
        it, k = divmod(j, K)
        if k == 0:
            start = margin.copy()
        if dist == "multinomial":
            ref = GR.softmax_pass(start, y, wobs, k, rate, SEED, it, b.row_base)
        else:
            ref = GR.grad_pass(start[0], y, wobs, dist, c.get("dist_kw"), rate, SEED, it, b.row_base)
        assert ref.exact == (dist in GR.EXACT)
        assert (r["w"] is None) == (wobs is None and rate >= 1.0)
        ratio = max(ratio, ref.compare(_np(r["g"]), _np(r["h"]), _np(r["w"]), f"tree {j}"))
        # j. the maxima behind the scales: of these arrays, or bounds they respect
        mx = np.array([np.abs(_np(r["g"])).max(), _np(r["h"]).max(), 1.0 if r["w"] is None else _np(r["w"]).max(),
                       0.0], np.float32)
        stat = _np(r["stat"]).view(np.float32)
        if r["fixed"]:
            assert stat.tolist() == [*GRAD_BOUNDS[dist], 0.0] and (mx <= stat).all(), (j, mx, stat)
        else:
            assert stat.tobytes() == mx.tobytes(), (j, mx, stat)
        assert b.max_rows_per_wg == Q.host_max_rows_per_wg(n, bm.F, nbt, segmented=b.segmented, cls=type(b))
        # a. scales from the maxima (or the fixed bounds) the tree was given
        want = Q.scales(_np(r["stat"]), p.mode, b.max_rows_per_wg)
        g, h, w = _np(r["g"]), _np(r["h"]), _np(r["w"])
        qscale, nid = _np(r["qscale"]), _np(r["nid"])
        tree = trees_from_bytes(_np(r["tree"]), b.capacity)[0]
        # c - f. the walk
        info = {}
        gpu_cat = None if r["cat"] is None else _np(r["cat"]).view(np.uint32).reshape(-1, 8)
        assert (gpu_cat is None) == (catf is None)
        ties.append(Q.verify(codes, nv, e, g, h, w, p, want, b.row_base, ti & 0x7FFFFFFF, _np(r["fmask"]), tree, nid,
                             qscale, tree_index=ti, catf=catf, gpu_cat=gpu_cat, info=info))
        infos.append(info)
        # the Newton re-derivation of the monotone intervals ran exactly where the oracle took it
        assert r["newton"] == int(info["newton"]), (j, r["newton"])
        # k. the ensemble keeps the tree's bitsets as the builder left them
        if catf is not None:
            kept = np.asarray(ens.catbits[j], np.uint32)
            m = min(len(kept), len(gpu_cat))
            assert m >= len(info["catbits"]) and np.array_equal(kept[:m], gpu_cat[:m]), f"tree {j}: ens.catbits"
        # b. the level-0 packed rows are the model's (scan engine)
        if not b.segmented:
            gq, sq = Q.quantised_rows(g, h, w, p.mode, want, b.row_base, ti & 0x7FFFFFFF)
            pk = r["pk"].view(torch.int32)[:n] if b.pk32 else r["pk"][:n]
            got = _np(pk).view(np.uint32 if b.pk32 else np.uint64)
            assert np.array_equal(got, Q.packed_rows(gq, sq, b.pk32)), f"tree {j}: packed rows"
            assert (gq != np.floor(g.astype(np.float64) * want[0])).any(), "dither had no effect"
        # g. margins: fp32 accumulation in tree order
        margin[j % K] += tree["value"][~nid.astype(np.int64)]
    got = ens._state.Fm[:, :n].cpu().numpy()
    assert got.tobytes() == margin.tobytes(), "training margins"
    print(f"{name}: near-tie nodes per tree {ties}; gradients worst err / tol {ratio:.3f}")
    # h.
    assert max(ties) <= 1, ties
    _verify_scoring(name, ens, bm, margin)
    if name in NEW_CASES:
        print(f"{name}: witnesses {case_witnesses(name, infos)}")
    return ties


def _verify_scoring(name, ens, bm, margin):
    """l. Scoring closes the chain: predict_raw_kernel on the raw training data
    and predict_binned_kernel on the device codes give the reconstructed
    margins bit for bit - both add the leaf values in tree order onto init_f
    in fp32, as step g does (DRF: onto zero).  This pins ``v <= thr`` against
    ``code <= bin`` on the real edges and cat_left against the trained bitsets.
    DRF's average is one more operation, the same one applied here to the
    reconstructed sums: an in-place division of the fp32 device tensor by the
    number of trees, so raw_margin is held bit for bit as well."""
    from h2omx import ops

    X = case_data(name)[0]
    n, K = bm.n, ens.K
    assert ens.average == (CASES[name]["dist"] == "drf") and margin.dtype == np.float32
    Xd = torch.tensor(X).cuda()
    raw = ens.raw_margin(Xd).cpu().numpy()
    want = margin
    if ens.average:
        avg = torch.from_numpy(margin.copy()).cuda()
        avg /= ens.ntrees
        want = avg.cpu().numpy()
    assert raw.tobytes() == want.tobytes(), f"{name}: raw_margin, {(raw != want).sum()} rows differ"
    _, nodes, cbits = ens._dev_nodes
    T = ens.trees.shape[0]
    assert (cbits is not None) == (case_catf(name) is not None)
    lib, P = ops.tree_lib(), ops.P
    roots = torch.arange(T, dtype=torch.int32, device=Xd.device) * ens.trees.shape[1]
    start = np.repeat((ens.init_f * (not ens.average)).astype(np.float32)[:, None], n, 1)
    out = torch.from_numpy(start).cuda()
    ops.check(lib.h2omx_predict_binned(P(bm.codes), bm.npad, n, P(nodes), P(roots), T, K, bm.nbt, P(out), out.stride(0),
                                       P(cbits), ops.stream(out.device)), "predict_binned")
    torch.cuda.synchronize()
    binned = out.cpu().numpy()
    assert binned.tobytes() == margin.tobytes(), f"{name}: predict_binned, {(binned != margin).sum()} rows differ"
    if ens.average:
        out = torch.from_numpy(start).cuda()
        ops.check(lib.h2omx_predict_raw(P(Xd), Xd.stride(0), n, P(nodes), P(roots), T, K, P(out), out.stride(0),
                                        P(cbits), ops.stream(out.device)), "predict_raw")
        torch.cuda.synchronize()
        sums = out.cpu().numpy()
        assert sums.tobytes() == margin.tobytes(), f"{name}: predict_raw sums, {(sums != margin).sum()} rows differ"


def test_scan_defaults(cuda_dev, monkeypatch):
    """bernoulli, fixed gradient bounds, bundled planes, int16 node ids, level prologues"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "scan_defaults")
    b = calls[0]["builder"]
    assert b.planes is not None and b.nid16 is not None and b.fuse_route and not b.segmented
    assert all(r["fixed"] and r["w"] is None for r in calls)
    _verify_all("scan_defaults", ens, bm, calls)
    assert any((t["na_left"][t["feat"] >= 0] == 1).any() for t in ens.trees), "no NA-left split"


def test_scan_every_switch_off(cuda_dev, monkeypatch):
    """gaussian with per-tree maxima; min_rows 400 makes early leaves"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "scan_switches_off")
    b = calls[0]["builder"]
    assert b.planes is None and not b.fuse_route and not b.pk32 and b.nid16 is None
    assert not any(r["fixed"] for r in calls)
    _verify_all("scan_switches_off", ens, bm, calls)
    t0, depth_of, stack = ens.trees[0], {}, [(0, 0)]
    while stack:
        i, d = stack.pop()
        depth_of[i] = d
        if t0[i]["feat"] >= 0:
            stack += [(int(t0[i]["left"]), d + 1), (int(t0[i]["left"]) + 1, d + 1)]
    depth = CASES["scan_switches_off"]["tp"]["max_depth"]
    assert any(t0[i]["feat"] < 0 and d < depth for i, d in depth_of.items()), "no early leaf"
    assert max(depth_of.values()) == depth


def test_xgboost_mode(cuda_dev, monkeypatch):
    """second-order gain on (G, H), lambda 1, min_child_weight 1, bagged rows of weight zero"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "xgb")
    assert all(r["w"] is not None and float((r["w"] == 0).float().mean()) > 0.2 for r in calls)
    _verify_all("xgb", ens, bm, calls)


def test_two_slot_passes(cuda_dev, monkeypatch):
    """depth 8 with one 64 KB histogram window: the last level takes two slot
    passes (parent-minus-sibling subtraction across passes)"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "two_slot_passes")
    b = calls[0]["builder"]
    assert b.plan_level(64)["passes"] > 1
    _verify_all("two_slot_passes", ens, bm, calls)


def test_packed_rows_32bit(cuda_dev, monkeypatch):
    """600 000 rows on 8 target workgroups: >= 2^16 rows per workgroup, 32-bit packed rows"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "pk32")
    b = calls[0]["builder"]
    assert b.pk32 and b.max_rows_per_wg >= 65536
    _verify_all("pk32", ens, bm, calls)


def test_multinomial(cuda_dev, monkeypatch):
    """three trees per iteration, each with its own class's maxima"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "multinomial")
    assert ens.K == 3
    stats = {r["stat"].cpu().numpy().tobytes() for r in calls}
    assert len(stats) > 1
    _verify_all("multinomial", ens, bm, calls)


def test_segmented_drf(cuda_dev, monkeypatch):
    """segmented engine: mean leaves, mtries 3, bagging with compacted root segment"""
    ens, bm, calls, direct = _train_spied(monkeypatch, "seg_drf")
    b = calls[0]["builder"]
    assert b.segmented and b.bag_compact and not direct
    _verify_all("seg_drf", ens, bm, calls)


@pytest.mark.parametrize("name,dmode", [("seg_drf_direct_wg", 2), ("seg_drf_direct_wave", 1)])
def test_segmented_drf_direct_levels(cuda_dev, monkeypatch, name, dmode):
    """direct levels from two nodes on: one workgroup per row chunk / one wave per node"""
    ens, bm, calls, direct = _train_spied(monkeypatch, name)
    assert calls[0]["builder"].segmented and set(direct) == {dmode}, set(direct)
    _verify_all(name, ens, bm, calls)


# ---- the gradient passes of the remaining distributions ------------------------

def test_poisson_weighted(cuda_dev, monkeypatch):
    """poisson on counts with observation weights: per-tree maxima of weighted rows"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "poisson_w")
    assert all(r["w"] is not None and not r["fixed"] and float(r["w"].max()) > 1.5 for r in calls)
    _verify_all("poisson_w", ens, bm, calls)


def test_gamma(cuda_dev, monkeypatch):
    """gamma on a positive response: h = y exp(-f) far from 1, per-tree maxima"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "gamma")
    assert all(r["w"] is None and not r["fixed"] for r in calls)
    assert float(calls[0]["h"].max()) > 4 * float(calls[0]["h"].median())
    _verify_all("gamma", ens, bm, calls)


def test_tweedie(cuda_dev, monkeypatch):
    """tweedie, power 1.2, 30 % zeros in the response"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "tweedie")
    assert all(r["w"] is None and not r["fixed"] for r in calls)
    _verify_all("tweedie", ens, bm, calls)


def test_laplace_fixed_bounds(cuda_dev, monkeypatch):
    """laplace: sign gradients under the fixed bounds, initial margin the median"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "laplace")
    assert all(r["fixed"] and r["w"] is None for r in calls)
    assert {float(v) for v in calls[0]["g"].unique()} <= {-1.0, 0.0, 1.0}
    _verify_all("laplace", ens, bm, calls)


def test_quantile_bagged_fixed_bounds(cuda_dev, monkeypatch):
    """quantile 0.3 with a 70 % bag: fixed bounds although w is a stream"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "quantile_bag")
    assert all(r["fixed"] and r["w"] is not None and 0.2 < float((r["w"] == 0).float().mean()) < 0.4 for r in calls)
    _verify_all("quantile_bag", ens, bm, calls)


def test_huber_weighted(cuda_dev, monkeypatch):
    """huber, delta 0.8, observation weights: both branches taken"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "huber_w")
    assert all(r["w"] is not None and not r["fixed"] for r in calls)
    r0 = (calls[0]["g"] / calls[0]["w"]).abs()
    assert 0.05 < float((r0 < 0.79).float().mean()) < 0.95
    _verify_all("huber_w", ens, bm, calls)


# ---- categorical set splits, monotone and interaction constraints ---------------

def _off_domain_walk(tree, bits, x, seen=None):
    """The leaf value of one raw row by the documented rule: NaN follows
    na_left; a categorical split truncates the value to a level code towards
    zero, so -0.5 is level 0 and 3.7 level 3; a code outside 0 .. 255 follows
    the NA direction, any other tests its bit; a numeric split compares
    v <= thr.  The project this one is modelled on holds no scorer, so nothing
    outside this repository decides the fractional case: the rule is pinned as
    predict_raw_kernel ((int)v) and the CPU scorer (reference.tree
    .predict_tree_numpy, astype(int64)) both implement it.  For +-inf and
    values of 2^31 and more the C++ cast is undefined; what is pinned there is
    what the gfx950 conversion instruction and this compiler make of it, a
    saturation to the int range and hence the NA direction."""
    i = 0
    while tree[i]["feat"] >= 0:
        nd, v = tree[i], float(x[int(tree[i]["feat"])])
        nal = bool(nd["na_left"] & 1)
        if math.isnan(v):
            left = nal
        elif nd["na_left"] & 2:
            b = math.trunc(v) if math.isfinite(v) else (1 << 31) * (1 if v > 0 else -1)
            left = nal if (b < 0 or b > 255) else bool((int(bits[i][b >> 5]) >> (b & 31)) & 1)
            if seen is not None:
                seen.add((i, b, nal))
        else:
            left = np.float32(v) <= nd["thr"]
        i = int(nd["left"]) + (0 if left else 1)
    return tree[i]["value"]


_ODD = np.array([256.0, 300.0, 1e9, -1.0, -7.0, 3.7, -0.5, 0.999, np.inf, -np.inf, np.nan, 255.0, 0.0, 2.0, 254.5,
                 255.999, -0.999, 2147483648.0], np.float32)


def _verify_off_domain(name, ens, bm):
    """Raw values no training row holds, in the categorical columns: levels of
    256 and more, negative values, non-integers, +-inf, NaN, and 255 (inside
    0 .. 255, in no left set: it tests its bit and goes right whatever the NA
    direction).  Every categorical split of every tree gets a training row that
    reaches it (found on the binned codes), with the split's column replaced by
    each odd value in turn, so 255 and the codes outside 0 .. 255 meet splits of
    both NA directions (the data sets give the NA rows a strong effect of their
    own: about ten categorical splits per case send NA left)."""
    X, codes = case_data(name)[0], case_data(name)[5]
    nbt, cols = bm.nbt, []
    for t in range(ens.trees.shape[0]):
        tr, bits = ens.trees[t], ens.catbits[t]
        parent = {}
        for i in reachable(tr):
            if tr[i]["feat"] >= 0:
                parent[int(tr[i]["left"])] = (i, True)
                parent[int(tr[i]["left"]) + 1] = (i, False)
        for i in [i for tt, i in _cat_splits(ens) if tt == t]:
            here, g = np.ones(X.shape[1], bool), i
            while g in parent:
                g, went_left = parent[g]
                nd = tr[g]
                c = codes[int(nd["feat"])].astype(np.int64)
                if nd["na_left"] & 2:
                    left = ((bits[g][np.minimum(c, 255) >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)
                else:
                    left = c <= nd["bin"]
                left = np.where(c == nbt - 1, bool(nd["na_left"] & 1), left)
                here &= left == went_left
            assert here.any(), f"node {i} of tree {t} holds no training row"
            col = np.repeat(X[:, np.nonzero(here)[0][:1]], _ODD.size, 1)
            col[int(tr[i]["feat"])] = _ODD
            cols.append(col)
    Xs = np.concatenate(cols, axis=1)
    assert not ens.average
    got = ens.raw_margin(torch.tensor(Xs).cuda()).cpu().numpy()
    want = np.repeat(ens.init_f.astype(np.float32)[:, None], Xs.shape[1], 1)
    seen = set()
    for t in range(ens.trees.shape[0]):
        for r in range(Xs.shape[1]):
            want[t % ens.K, r] += _off_domain_walk(ens.trees[t], ens.catbits[t], Xs[:, r], seen)
    # the walk met what it is for: 255 and the codes outside 0 .. 255 at splits of
    # both NA directions (a row whose ancestors split on the same column may leave its path)
    for b in (255, 256, -1, 1 << 31, -(1 << 31)):
        assert {nal for _, bb, nal in seen if bb == b} == {False, True}, (b, sorted(seen)[:8])
    assert {0, 2, 3, 254} <= {bb for _, bb, _ in seen}
    bad = got != want
    assert not bad.any(), (name, np.argwhere(bad).tolist()[:10], Xs[:, bad.any(0)][:, :5])


def _cat_splits(ens):
    """(tree, node id) of every reachable categorical split"""
    return [(t, i) for t in range(ens.trees.shape[0]) for i in reachable(ens.trees[t])
            if ens.trees[t][i]["feat"] >= 0 and ens.trees[t][i]["na_left"] & 2]


def test_categorical_gaussian(cuda_dev, monkeypatch):
    """NBT 64 (one bin per lane): a 37-level column with 3 % NA, a 5-level one,
    continuous ones; left sets with gaps, NA left, numeric splits below"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "cat_gauss")
    b = calls[0]["builder"]
    assert bm.nbt == 64 and b.catf is not None and not b.segmented
    _verify_all("cat_gauss", ens, bm, calls)
    assert len(_cat_splits(ens)) > 10
    _verify_off_domain("cat_gauss", ens, bm)


def test_categorical_bernoulli_256(cuda_dev, monkeypatch):
    """NBT 256 (four bins per lane): 200 levels, bagged rows; left sets across
    bitset words, levels without mass in a node"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "cat_bern_256")
    assert bm.nbt == 256 and all(r["w"] is not None for r in calls)
    _verify_all("cat_bern_256", ens, bm, calls)
    words = {w for t, i in _cat_splits(ens) for w in np.nonzero(ens.catbits[t][i])[0].tolist()}
    assert len(words) >= 5, words
    _verify_off_domain("cat_bern_256", ens, bm)


def test_categorical_segmented_drf(cuda_dev, monkeypatch):
    """segmented engine with mtries: categorical features keep the levels on the
    subtraction path (no direct level although DIRECT_MIN_NODES is 2)"""
    ens, bm, calls, direct = _train_spied(monkeypatch, "cat_seg_drf")
    b = calls[0]["builder"]
    assert b.segmented and b.catf is not None and b.DIRECT_MIN_NODES == 2 and not direct
    _verify_all("cat_seg_drf", ens, bm, calls)
    assert len(_cat_splits(ens)) > 10


@pytest.mark.parametrize("name", ["mono_sqerr", "mono_newton", "mono_xgb"])
def test_monotone(cuda_dev, monkeypatch, name):
    """mono_ok in the scan, the level's intervals and clamps; squared-error
    splits with Newton leaves (gaussian and bernoulli) re-derive the intervals
    in mono_newton_kernel, XGBoost mode keeps the level's"""
    ens, bm, calls, _ = _train_spied(monkeypatch, name)
    b = calls[0]["builder"]
    assert b.gbound is not None and not b.segmented
    assert [r["newton"] for r in calls] == [int(name != "mono_xgb")] * len(calls)
    _verify_all(name, ens, bm, calls)


def test_interaction_scan(cuda_dev, monkeypatch):
    """interaction sets (0, 1), (2, 3) and an unlisted feature: inter_ok and the
    istate handed to the children"""
    ens, bm, calls, _ = _train_spied(monkeypatch, "inter_scan")
    assert calls[0]["builder"].istate is not None
    _verify_all("inter_scan", ens, bm, calls)


def test_interaction_segmented_deep(cuda_dev, monkeypatch):
    """depth 12 on the segmented engine: the last level has 2048 potential
    nodes and runs direct (inter_ok in the direct scans)"""
    ens, bm, calls, direct = _train_spied(monkeypatch, "inter_seg_deep")
    assert calls[0]["builder"].segmented and direct, direct
    _verify_all("inter_seg_deep", ens, bm, calls)


# ---- the split scan on histograms of our own ---------------------------------

_FEAT_BEST = np.dtype([("gain", "<f8"), ("GL", "<f8"), ("SL", "<f8"), ("G", "<f8"), ("S", "<f8"), ("pad0", "<f8"),
                       ("code", "<i4"), ("pad1", "<i4"), ("pad2", "<f8")])


def _synthetic_level(nbt, seed):
    """Four nodes of a level, children of two parents: random int64 (G, S)
    rows with empty bins (exact ties between neighbouring thresholds), NA mass
    in some rows, and - what no binned matrix can hold - mass in bins at and
    past nvb[f], placed so that the threshold t = nvb[f] would be the best
    split of (node 0, feature 1) and (node 1, feature 2) were it a candidate."""
    rng = np.random.default_rng(seed)
    F = 6
    nvb = np.array([nbt - 1, nbt * 2 // 5, 7, 3, 1, nbt * 3 // 4], np.int32)
    S = rng.integers(1, 3000, (4, F, nbt))
    S[rng.random(S.shape) < 0.4] = 0
    G = np.where(S > 0, rng.integers(-(1 << 18), 1 << 18, S.shape), 0)
    for f in range(F):
        G[:, f, nvb[f]:] = 0
        S[:, f, nvb[f]:] = 0
    for node, f in ((0, 1), (2, 1), (1, 3), (3, 3), (0, 0)):       # NA mass
        G[node, f, nbt - 1], S[node, f, nbt - 1] = -70000, 2500
    for node, f in ((0, 1), (1, 2)):
        m = int(nvb[f])
        G[node, f, :m] //= 64
        G[node, f, m], S[node, f, m] = -(1 << 22), 40000
        G[node, f, m + 1], S[node, f, m + 1] = 1 << 22, 40000
    return G.astype(np.int64), S.astype(np.int64), nvb


@pytest.mark.parametrize("mode", [0, 1], ids=["gbm", "xgb"])
@pytest.mark.parametrize("nbt", [256, 64, 32])
def test_split_scan_on_synthetic_histograms(cuda_dev, nbt, mode):
    """h2omx_split_find (feat_best_wave + feat_scan_wave) on a level whose
    histograms the test writes itself, against the oracle's per-feature
    records, to the bit: built rows and parent-minus-sibling rows, the NA bin,
    both NA directions, ties between thresholds, a masked feature, and the
    last valid bin.  The binning only emits codes below nvb[f], so in a
    trained tree a scan over t <= nvb[f] merely repeats the last valid
    threshold and loses the tie on its code; the rule "t < min(nvb[f], nbt -
    1)" shows only where bins past nvb[f] hold mass, as they do here."""
    import ctypes

    from h2omx import ops
    from h2omx.models.tree import TreeParams
    from h2omx.models.tree.structs import SplitParams

    G, S, nvb = _synthetic_level(nbt, 40 + nbt + mode)
    n_nodes, F, _ = G.shape
    ig, is_ = 2.0 ** -12, 2.0 ** -8
    p = TreeParams(mode=mode, min_rows=6.0, min_child_weight=6.0 if mode else 0.0,
                   reg_lambda=1.0 if mode else 0.0, reg_alpha=0.25 if mode else 0.0, gamma=0.0)
    fmask = np.array([1, 1, 1, 1, 0, 1], np.uint8)
    want = Q.LevelScan(G, S, nvb, p, ig, is_, np.broadcast_to(fmask.astype(bool), (n_nodes, F)))
    # the trap is armed: one more threshold would win both planted rows
    wider = Q.LevelScan(G, S, nvb + np.array([0, 1, 1, 0, 0, 0], np.int32), p, ig, is_,
                        np.broadcast_to(fmask.astype(bool), (n_nodes, F)))
    for node, f in ((0, 1), (1, 2)):
        assert wider.f_gain[node, f] > want.f_gain[node, f] > 0 and wider.f_code[node, f] >> 1 == nvb[f]
        assert want.f_code[node, f] >> 1 < nvb[f]
    assert (want.f_code[want.f_gain > -np.inf] & 1).any(), "no NA-left winner"

    dev = cuda_dev
    hist = np.stack([G, S], axis=2)                               # [node][F][2][nbt]
    built = torch.from_numpy(np.ascontiguousarray(hist[[0, 3]])).to(dev)
    parents = torch.from_numpy(np.ascontiguousarray(np.stack([hist[0] + hist[1], hist[2] + hist[3]]))).to(dev)
    full = torch.zeros((n_nodes, F, 2, nbt), dtype=torch.int64, device=dev)
    link = torch.tensor([[0, -1, 0, 0], [-1, 0, 0, 0], [-1, 1, 1, 0], [1, -1, 1, 0]], dtype=torch.int32, device=dev)
    ctl = torch.tensor([n_nodes, 2, 3, 3 + n_nodes], dtype=torch.int32, device=dev)
    qscale = torch.zeros(16, dtype=torch.float64, device=dev)
    qscale[2], qscale[3] = ig, is_
    out = torch.zeros(n_nodes * F * _FEAT_BEST.itemsize, dtype=torch.uint8, device=dev)
    sp = SplitParams()
    sp.mode, sp.F, sp.min_rows, sp.min_child_weight = mode, F, p.min_rows, p.min_child_weight
    sp.lambda_, sp.alpha, sp.gamma, sp.col_rate, sp.depth = p.reg_lambda, p.reg_alpha, p.gamma, 1.0, 2
    lib, P = ops.tree_lib(), ops.P
    nvb_d, fmask_d = torch.from_numpy(nvb).to(dev), torch.from_numpy(fmask).to(dev)
    ops.check(lib.h2omx_split_find(P(built), P(parents), P(full), P(ctl), P(link), P(nvb_d), P(fmask_d), P(qscale),
                                   ctypes.addressof(sp), n_nodes, nbt, P(out), ops.stream(dev)), "split_find")
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(_FEAT_BEST).reshape(n_nodes, F)
    assert np.array_equal(full.cpu().numpy(), hist), "completed histogram rows"
    for fld, ref in (("code", want.f_code), ("gain", want.f_gain), ("GL", want.f_GL), ("SL", want.f_SL),
                     ("G", want.f_G), ("S", want.f_S)):
        ref = ref.astype(got[fld].dtype)
        same = got[fld].view(np.int64 if fld != "code" else np.int32) == ref.view(np.int64 if fld != "code" else np.int32)
        assert same.all(), (fld, np.argwhere(~same).tolist(), got[fld][~same], ref[~same])


@pytest.mark.parametrize("mode", [0, 1], ids=["gbm", "xgb"])
@pytest.mark.parametrize("nbt,nvb_cat", [(256, 255), (256, 37), (64, 37), (64, 255), (128, 100), (32, 2)])
def test_categorical_scan_on_synthetic_histograms(cuda_dev, nbt, nvb_cat, mode):
    """h2omx_split_find with categorical rows (the CAT instantiation of every
    NBT: feat_best_cat_wave, and the threshold scan for the numeric row beside
    them) on oracle_cases.cat_level, against the oracle: the FeatBest records
    and the eight left-set words of every (node, feature) bit for bit.  What
    no trained tree reaches together: levels of equal key, mass past nvb[f],
    255 levels, a left set filling word 7, a row with one level, a masked
    categorical feature.  Every feature carries a monotone sign: the numeric
    row's candidates go through mono_ok, the categorical rows' do not."""
    import ctypes

    from h2omx import ops
    from h2omx.models.tree import TreeParams
    from h2omx.models.tree.structs import SplitParams
    from oracle_cases import cat_level

    G, S, nvb = cat_level(nbt, nvb_cat, True, 90 + nbt + nvb_cat + mode, numeric_row=True)
    n_nodes, F, _ = G.shape
    ig, is_ = 2.0 ** -12, 2.0 ** -8
    p = TreeParams(mode=mode, min_rows=6.0, min_child_weight=6.0 if mode else 0.0, learn_rate=0.1,
                   reg_lambda=1.0 if mode else 0.0, reg_alpha=0.25 if mode else 0.0, gamma=0.0)
    catf = np.array([1, 1, 1, 0], np.uint8)
    mono = np.array([1, -1, 1, -1], np.int8)
    fmask = np.array([1, 1, 0, 1], np.uint8)
    allowed = np.broadcast_to(fmask.astype(bool), (n_nodes, F))
    want = Q.LevelScan(G, S, nvb, p, ig, is_, allowed, catf.astype(bool), mono.astype(np.int64))
    free = Q.LevelScan(G, S, nvb, p, ig, is_, allowed, catf.astype(bool))
    assert np.array_equal(want.f_code[:, :3], free.f_code[:, :3])
    removed = (want.gains[:, 3] == -np.inf) & (free.gains[:, 3] > -np.inf)
    assert removed.any() and not removed.all(), "mono_ok: some candidates of the numeric row, not all"
    has = want.f_gain > -np.inf
    assert has[:4, 1].all() and has[:, 0].sum() >= 3 and not has[:, 2].any() and (want.f_code[has] & 1).any()
    bits = np.zeros((n_nodes, F, 8), np.uint32)
    for i, f in zip(*np.nonzero(has[:, :3])):
        bits[i, f] = Q.bitset(want.left_set(i, int(f), int(want.f_code[i, f]) >> 1))
    if (nbt, nvb_cat) == (256, 255):
        assert bits[3, 0, 7] == 0x7FFFFFFF, "word 7 not filled"

    dev = cuda_dev
    hist = np.ascontiguousarray(np.stack([G, S], axis=2))          # [node][F][2][nbt], every node built in its slot
    built = torch.from_numpy(hist).to(dev)
    parents = torch.zeros((1, F, 2, nbt), dtype=torch.int64, device=dev)
    full = torch.zeros((n_nodes, F, 2, nbt), dtype=torch.int64, device=dev)
    link = torch.tensor([[i, -1, 0, 0] for i in range(n_nodes)], dtype=torch.int32, device=dev)
    ctl = torch.tensor([n_nodes, n_nodes, 7, 7 + n_nodes], dtype=torch.int32, device=dev)
    qscale = torch.zeros(16, dtype=torch.float64, device=dev)
    qscale[2], qscale[3] = ig, is_
    out = torch.zeros(n_nodes * F * _FEAT_BEST.itemsize, dtype=torch.uint8, device=dev)
    fbcat = torch.full((n_nodes * F * 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    catf_d, mono_d = torch.from_numpy(catf).to(dev), torch.from_numpy(mono).to(dev)
    sp = SplitParams()
    sp.mode, sp.leaf_mode, sp.F, sp.min_rows, sp.min_child_weight = mode, 0, F, p.min_rows, p.min_child_weight
    sp.lambda_, sp.alpha, sp.gamma, sp.col_rate, sp.depth = p.reg_lambda, p.reg_alpha, p.gamma, 1.0, 3
    sp.learn_rate, sp.max_abs_leaf = p.learn_rate, 0.0
    sp.catf, sp.fbcat, sp.mono = catf_d.data_ptr(), fbcat.data_ptr(), mono_d.data_ptr()
    lib, P = ops.tree_lib(), ops.P
    nvb_d, fmask_d = torch.from_numpy(nvb).to(dev), torch.from_numpy(fmask).to(dev)
    ops.check(lib.h2omx_split_find(P(built), P(parents), P(full), P(ctl), P(link), P(nvb_d), P(fmask_d), P(qscale),
                                   ctypes.addressof(sp), n_nodes, nbt, P(out), ops.stream(dev)), "split_find")
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(_FEAT_BEST).reshape(n_nodes, F)
    assert np.array_equal(full.cpu().numpy(), hist), "completed histogram rows"
    for fld, ref in (("code", want.f_code), ("gain", want.f_gain), ("GL", want.f_GL), ("SL", want.f_SL),
                     ("G", want.f_G), ("S", want.f_S)):
        ref = ref.astype(got[fld].dtype)
        same = got[fld].view(np.int64 if fld != "code" else np.int32) == ref.view(np.int64 if fld != "code" else np.int32)
        assert same.all(), (fld, np.argwhere(~same).tolist(), got[fld][~same], ref[~same])
    # allowed categorical rows write their eight words (zeros without a winner);
    # the numeric row and the masked feature leave the scratch alone
    words = fbcat.cpu().numpy().view(np.uint32).reshape(n_nodes, F, 8)
    assert (words[:, 2:] == 0x5A5A5A5A).all(), "bitsets written for a masked / numeric row"
    same = words[:, :2] == bits[:, :2]
    assert same.all(), ("fbcat", np.argwhere(~same).tolist(), words[:, :2][~same], bits[:, :2][~same])
