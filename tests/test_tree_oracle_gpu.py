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
poisson_w, gamma, tweedie, laplace, quantile_bag and huber_w: 0 in all 18."""
import copy

import numpy as np
import pytest
import torch

import gradref as GR
import quantref as Q
from oracle_cases import CASES, case_data, case_weights, tree_params
from h2omx.models.tree import bin_matrix, train_ensemble
from h2omx.models.tree.engine import GRAD_BOUNDS, trees_from_bytes

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
    bm = bin_matrix(torch.tensor(X).cuda(), e.copy(), nv.copy(), nbt)
    calls, direct_modes = [], []
    build = E.HipTreeBuilder.build

    def spy(self, g, h, w, tree_index, tree_fmask=None, grad_fuse=None, stat=None, chain=False):
        assert grad_fuse is None and not chain
        n = self.bm.n
        rec = dict(builder=self, tree_index=tree_index, p=copy.copy(self.p), g=g[:n].clone(), h=h[:n].clone(),
                   w=None if w is None else w[:n].clone(),
                   fmask=None if tree_fmask is None else tree_fmask.clone(),
                   stat=(self.stat_max if stat is None else stat).clone(), fixed=stat is not None)
        out = build(self, g, h, w, tree_index, tree_fmask, grad_fuse, stat, chain)
        rec.update(tree=out.clone(), qscale=self.qscale.clone(), nid=self.nid[:n].clone(), pk=self.pk.clone())
        calls.append(rec)
        return out

    monkeypatch.setattr(E.HipTreeBuilder, "build", spy)
    lib = ops.tree_lib()
    seg_direct = lib.h2omx_seg_direct

    def spy_direct(*a):
        direct_modes.append(a[15])     # dmode: 0 workgroup per node, 1 wave per node, 2 workgroup per row chunk
        return seg_direct(*a)

    monkeypatch.setattr(lib, "h2omx_seg_direct", spy_direct)
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
    ties, ratio = [], 0.0
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
        ties.append(Q.verify(codes, nv, e, g, h, w, p, want, b.row_base, ti & 0x7FFFFFFF, _np(r["fmask"]), tree, nid,
                             qscale, tree_index=ti))
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
    return ties


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
