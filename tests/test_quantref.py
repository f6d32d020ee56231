"""CPU tests of the fixed-point tree oracle (tests/quantref.py): its scan, tie
and partition logic against the independent float64 reference builder on
inputs both compute exactly, the quantisation model's statistical properties,
the fixed-point headroom of the packed adds, and how often the data sets of
the GPU oracle tests produce near-ties."""
import math

import numpy as np
import pytest
import torch

import quantref as Q
from oracle_cases import CASES, builder_class, case_data, case_weights, tree_params
from h2omx.models.tree import TreeParams, bin_matrix, compute_edges
from h2omx.reference.tree import RefTreeBuilder, bag_weights, dist_grad
from treecmp import reachable


# ---- integer inputs: both builders are exact --------------------------------

def _int_data():
    rng = np.random.default_rng(5)
    n, F = 6000, 7
    X = rng.normal(size=(F, n)).astype(np.float32)
    X[2, rng.random(n) < 0.1] = np.nan
    X[5] = rng.integers(0, 4, n)
    sig = 2.0 * X[0] - 1.5 * X[1] * X[3] + 2.0 * np.nan_to_num(X[2], nan=-1.5) + 1.2 * X[5] - 1.8
    g = np.clip(np.rint(sig + rng.normal(size=n)), -8, 8).astype(np.float32)
    return X, g


_int_cache = {}


def _int_case(nbins):
    if nbins not in _int_cache:
        X, g = _int_cache.setdefault("data", _int_data())
        Xt = torch.from_numpy(X)
        e, nv, nbt = compute_edges(Xt, nbins)
        _int_cache[nbins] = (bin_matrix(Xt, e, nv, nbt), g)
    return _int_cache[nbins]


@pytest.mark.parametrize("min_rows", [10, 400])
@pytest.mark.parametrize("mode", [0, 1], ids=["gbm", "xgb"])
@pytest.mark.parametrize("nbins", [255, 63, 20])
def test_integer_inputs_match_reference_builder(nbins, mode, min_rows):
    """integer g in [-8, 8], h = w = 1, every scale 1 and no dither: the sums
    of both builders are exact, so the trees agree field by field"""
    bm, g = _int_case(nbins)
    n = bm.n
    # (mode 1 bounds the children by min_child_weight on H = the row count here)
    p = TreeParams(max_depth=5, min_rows=min_rows, min_child_weight=min_rows if mode else 0.0, mode=mode,
                   reg_lambda=1.0 if mode else 0.0)
    ref = RefTreeBuilder(bm, p)
    ref.nid[:] = -1
    ref.nid[:n] = 0
    pad = np.zeros(bm.npad - n, np.float32)
    ones = np.ones(n, np.float32)
    want = ref.build(np.concatenate([g, pad]), np.concatenate([ones, pad]), np.concatenate([ones, pad]), 0)
    codes = bm.codes.numpy()[:, :n]
    got, leaf, records = Q.grow(codes, bm.nvb.numpy(), bm.edges.numpy(), g, ones, ones, p, Q.unit_scales(), 0, 0,
                                dither=False)
    keep = reachable(want)
    assert keep == reachable(got)
    assert len(keep) > (3 if min_rows == 400 else 15), "degenerate tree"
    for fld in ("feat", "bin", "na_left", "left", "thr", "gain", "weight", "value"):
        assert want[keep][fld].tobytes() == got[keep][fld].tobytes(), (fld, want[keep][fld], got[keep][fld])
    assert np.array_equal(leaf, ~ref.nid[:n])
    if nbins == 255 and min_rows == 10:
        assert (want[keep]["na_left"] == 1).any() and (want[keep]["feat"] == 5).any()


def test_verify_reports_a_wrong_node():
    """verify walks a tree the oracle grew itself without complaint and names
    the node and field of a planted error"""
    bm, g = _int_case(63)
    n = bm.n
    p = TreeParams(max_depth=4, min_rows=10)
    ones = np.ones(n, np.float32)
    stat = np.array([8.0, 1.0, 1.0, 0.0], np.float32).view(np.int32)
    qs = Q.scales(stat, 0, 4096)
    args = (bm.codes.numpy()[:, :n], bm.nvb.numpy(), bm.edges.numpy(), g, ones, ones, p, qs, 0, 7, None)
    tree, leaf, _ = Q.grow(*args)
    full = np.zeros(31, tree.dtype)
    full[: len(tree)] = tree
    qscale = np.zeros(16)
    qscale[:7], qscale[9] = qs, 7
    assert Q.verify(*args, full, ~leaf, qscale) <= 1
    inner = [i for i in reachable(tree) if tree[i]["feat"] >= 0 and tree[i]["bin"] > 0][-1]
    bad = full.copy()
    bad["bin"][inner] -= 1
    with pytest.raises(Q.Mismatch, match=rf"gid {inner}\) field feat/bin/na_left"):
        Q.verify(*args, bad, ~leaf, qscale)
    moved = ~leaf.copy()
    moved[17] = ~int(tree[0]["left"])
    with pytest.raises(Q.Mismatch, match="row routing: 1 rows differ, first row 17"):
        Q.verify(*args, full, moved, qscale)
    with pytest.raises(Q.Mismatch, match=r"qscale\[0\]"):
        Q.verify(*args, full, ~leaf, np.concatenate([[qs[0] * 2], qscale[1:]]))


# ---- the quantisation model --------------------------------------------------

@pytest.mark.parametrize("gmax,rows_per_wg", [(1.0, 4096), (0.731, 65536), (37.5, 16)])
def test_quantisation_model_properties(gmax, rows_per_wg):
    n = 200_000
    rng = np.random.default_rng(3)
    g = rng.uniform(-gmax, gmax, n).astype(np.float32)
    stat = np.array([np.abs(g).max(), 1.0, 1.0, 0.0], np.float32).view(np.int32)
    sg, ss = Q.scales(stat, 0, rows_per_wg)[:2]
    rows = np.arange(n, dtype=np.int64) + (1 << 33) - n // 2       # row ids on both sides of 2^32 ... 2^33
    gq, sq = Q.quantise(g, np.ones(n, np.float32), sg, ss, rows, 11)
    x = g.astype(np.float64) * sg
    lo = np.floor(x).astype(np.int64)
    assert ((gq == lo) | (gq == lo + 1)).all()
    assert (gq != lo).any() and (gq == lo).any()
    # unbiased: 6 sigma of the mean of n uniform rounding errors, + 2^-9 for the
    # fp32 rounding of k + d once k >= 2^15
    assert abs((gq - x).mean()) <= 6 / math.sqrt(12 * n) + 2.0 ** -9
    # s = 1: ss + d2, which fp32 rounds up to ss + 1 when ss = 2^16 (steps of 2^-7) and d2 is near 1
    assert ss >= 1 and ((sq == int(ss)) | (sq == int(ss) + 1)).all() and (sq == int(ss)).mean() > 0.99
    again, _ = Q.quantise(g, np.ones(n, np.float32), sg, ss, rows, 11)
    other, _ = Q.quantise(g, np.ones(n, np.float32), sg, ss, rows, 12)
    assert np.array_equal(gq, again)
    assert 0.1 < (gq != other).mean() < 0.9
    # the high word of the row id reaches the hash
    shifted, _ = Q.quantise(g, np.ones(n, np.float32), sg, ss, rows + (1 << 32), 11)
    assert 0.1 < (gq != shifted).mean() < 0.9


def test_row_hash_known_values():
    """mix32 is a bijection with mix32(0) = 0, so row 0 under salt 0 hashes to 0;
    the hash takes the row id modulo 2^32 in its first operand only"""
    assert int(Q.row_hash(np.array([0]), 0)[0]) == 0
    h = Q.row_hash(np.array([5, 5 + (1 << 32)]), 9)
    assert h[0] != h[1] and int(h[1]) == int(Q.row_hash(np.array([5]), 10)[0])


# ---- fixed-point headroom ----------------------------------------------------

def _stat_values():
    """maxima across the mantissa range and many exponents: every scale the formulas produce"""
    out = []
    for e in (-20, -3, -1, 0, 1, 5, 17):
        for m in (1.0, 1.0 + 2.0 ** -23, 1.25, 1.5, 2.0 - 2.0 ** -23):
            out.append(np.float32(m * 2.0 ** e))
    return out


@pytest.mark.parametrize("rows_per_wg", [16, 4096, 65536, 262144])
def test_packed_add_headroom(rows_per_wg):
    qg, qsr = Q.row_ranges(rows_per_wg)
    assert rows_per_wg * (min(qg, Q.QG) + 1) < 2 ** 31
    assert rows_per_wg * (min(qsr, Q.QS) + 1) < 2 ** 32
    rng = np.random.default_rng(1)
    rows = rng.integers(0, 1 << 40, 4096)
    for mx in _stat_values():
        for mode in (0, 1):
            stat = np.array([mx, mx, mx, 0.0], np.float32).view(np.int32)
            qs = Q.scales(stat, mode, rows_per_wg)
            for j in (0, 1, 4, 5, 6):
                assert math.frexp(qs[j])[0] == 0.5, "scales are powers of two"
            assert qs[0] * mx <= min(qg, Q.QG) < 2 * qs[0] * mx
            assert qs[1] * mx <= min(qsr, Q.QS) < 2 * qs[1] * mx
            assert qs[4] * mx <= Q.LEAF_RANGE
            full = np.full(rows.size, mx, np.float32)
            for sign in (1.0, -1.0):
                gq, sq = Q.quantise(sign * full, full, qs[0], qs[1], rows, 3)
                # a workgroup chunk's sums stay inside the packed 31 / 32-bit fields
                assert np.abs(gq).max() <= min(qg, Q.QG) + 1 and sq.max() <= min(qsr, Q.QS) + 1 and sq.min() >= 0
                if rows_per_wg >= 65536:
                    # 16-bit fields of the 32-bit packed row cannot wrap
                    assert np.abs(gq).max() <= 2 ** 14 + 1 and sq.max() <= 2 ** 15 + 1
                    pk = Q.packed_rows(gq, sq, True)
                    assert np.array_equal(pk.astype(np.int32) >> 16, gq) and np.array_equal(pk & 0xFFFF, sq)


def test_level_plans_bound_the_chunks():
    """the host-side level plans, exercised on a bare builder as in
    test_builder_without_plane_count_plans_on_features: every plan's workgroup
    chunk is at most max_rows_per_wg, which the scales are derived from"""
    from h2omx.models.tree.engine import HipTreeBuilder

    class Narrow(HipTreeBuilder):
        TARGET_WGS = 8

    for cls, n, F, nbt in ((HipTreeBuilder, 20037, 7, 256), (HipTreeBuilder, 20037, 7, 64),
                           (HipTreeBuilder, 11_000_000, 28, 256), (Narrow, 600_000, 9, 256)):
        m = Q.host_max_rows_per_wg(n, F, nbt, cls=cls)
        assert 16 <= m <= HipTreeBuilder.ROWS_CAP
        b = cls.__new__(cls)
        b.F, b.nbt, b.max_rows_per_wg = F, nbt, m
        units = -(-n // 64) * 64 // 16
        for slots in (1, 2, 4, 16, 64, 128):
            plan = b._choose(slots, units)
            assert 16 * math.ceil(units / plan["wgpg"]) <= m, (n, slots, plan)
        qg, qsr = Q.row_ranges(m)
        assert m * (min(qg, Q.QG) + 1) < 2 ** 31 and m * (min(qsr, Q.QS) + 1) < 2 ** 32
        if cls is Narrow:
            assert m >= 65536, "the 32-bit packed-row case needs >= 2^16 rows per workgroup"
        elif n == 20037:
            assert m < 65536


# ---- near-tie audit ------------------------------------------------------------

def cpu_boost(name, trees_out=None):
    """The case's boosting run with the oracle as the tree builder (float64
    gradients from the reference; the audit counts near-ties, it does not
    compare with the GPU): near-tie nodes per tree."""
    from h2omx.models.tree.boost import _tree_fmask, init_margin, weighted_quantile
    from h2omx.models.tree.engine import GRAD_BOUNDS

    c = CASES[name]
    X, y, e, nv, nbt, codes = case_data(name)
    F, n = codes.shape
    p = tree_params(name)
    dist, K = c["dist"], (c.get("nclass", 1) if c["dist"] == "multinomial" else 1)
    rate, seed = c.get("sample_rate", 1.0), 3
    wobs, dist_kw = case_weights(name), c.get("dist_kw", {})
    m = Q.host_max_rows_per_wg(n, F, nbt, segmented=c["engine"] == "seg", cls=builder_class(name))
    if dist in ("laplace", "quantile"):
        q = 0.5 if dist == "laplace" else dist_kw.get("quantile_alpha", 0.5)
        init = np.array([weighted_quantile(y, None if wobs is None else torch.from_numpy(wobs), q)])
    else:
        init = init_margin(dist, y, wobs, K)
    Fm = np.repeat(init[:, None], n, 1).astype(np.float32)
    # bounded gradients of unweighted rows quantise with the bound scales (GpuBooster._bounds)
    fixed = K == 1 and wobs is None and dist in GRAD_BOUNDS
    counts = []
    for t in range(c["ntrees"]):
        wb = bag_weights(n, rate, seed, t)
        if wobs is not None:
            wb = wobs * wb
        if K == 1:
            grads = [dist_grad(dist, Fm[0], y, **dist_kw)]
        else:
            z = np.exp(Fm - Fm.max(axis=0, keepdims=True))
            pr = z / z.sum(axis=0, keepdims=True)
            grads = [(pr[k] - (y == k), np.maximum(pr[k] * (1 - pr[k]), 1e-16)) for k in range(K)]
        for k in range(K):
            g, h = ((v * wb).astype(np.float32) for v in grads[k])
            w = wb if (rate < 1.0 or wobs is not None) else None
            mx = GRAD_BOUNDS[dist] if fixed else (np.abs(g).max(), h.max(), 1.0 if w is None else w.max())
            qs = Q.scales(np.array([*mx, 0.0], np.float32).view(np.int32), p.mode, m)
            tree, leaf, rec = Q.grow(codes, nv, e, g, h, w, p, qs, 0, t * K + k, _tree_fmask(p, F, t, None))
            Fm[k] += tree["value"][leaf]
            counts.append(Q.near_tie_nodes(rec))
            if trees_out is not None:
                trees_out.append(tree)
    return counts


@pytest.mark.parametrize("name", list(CASES))
def test_near_tie_audit(name):
    """At most one near-tie node per tree on every data set of the GPU oracle
    tests (the gain has nothing for the compiler to contract, so the expected
    count is zero).  Observed near-tie nodes per tree: 0 for every tree of every
    case.  (Counted by :meth:`quantref.LevelScan.near`: before a candidate and
    its mirror image counted once, the depth-8 case showed 2 per tree - "all
    non-NA left" against "one bin and NA left" of a 3-valued column, the same
    partition with the sides exchanged, hence the same gain to the bit.)"""
    trees = []
    counts = cpu_boost(name, trees)
    print(name, "near-tie nodes per tree:", counts)
    assert max(counts) <= 1, counts
    # the audit is of real trees
    depth = CASES[name]["tp"]["max_depth"]
    assert all(len(t) > 4 * depth for t in trees), [len(t) for t in trees]
