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
from oracle_cases import (CASES, NEW_CASES, builder_class, case_catf, case_data, case_weights, case_witnesses,
                          cat_level, tree_params)
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


# ---- categorical scan: the vectorised model against a plain loop -----------------

def _plain_gain(GL, SL, G, S, p):
    """split_gain of one candidate on Python floats, or None when inadmissible"""
    GR, SR = G - GL, S - SL
    floor = p.min_rows if p.mode == 0 else p.min_child_weight
    if SL < floor or SR < floor or SL <= 0.0 or SR <= 0.0:
        return None
    if p.mode == 0:
        return GL * GL / SL + GR * GR / SR - G * G / S

    def t(x):
        a = p.reg_alpha
        if a <= 0.0:
            return x
        return x - a if x > a else (x + a if x < -a else 0.0)

    lam = p.reg_lambda
    return 0.5 * (t(GL) * t(GL) / (SL + lam) + t(GR) * t(GR) / (SR + lam) - t(G) * t(G) / (S + lam)) - p.gamma


def plain_cat_best(G, S, nvb_f, nbt, ig, is_, p):
    """feat_best_cat_wave of one (node, feature) row, level by level: (gain,
    code, GL, SL, left levels) of the winner, or None.  G, S: lists of ints."""
    T = nbt - 1
    levels = [b for b in range(min(nvb_f, T)) if S[b] > 0]
    levels.sort(key=lambda b: (float(G[b]) / float(S[b]), b))
    tg, ts = float(sum(G)) * ig, float(sum(S)) * is_
    ng, ns = float(G[T]) * ig, float(S[T]) * is_
    best, cg, cs = None, 0, 0
    for r, b in enumerate(levels):
        cg, cs = cg + G[b], cs + S[b]
        for na in (0, 1):
            if na and not ns > 0.0:
                continue
            GL, SL = float(cg) * ig, float(cs) * is_
            if na:
                GL, SL = GL + ng, SL + ns
            gain = _plain_gain(GL, SL, tg, ts, p)
            if gain is None or not gain > -math.inf:
                continue
            code = 2 * b + na
            if best is None or gain > best[0] or (gain == best[0] and code < best[1]):
                best = (gain, code, GL, SL, sorted(levels[: r + 1]))
    return best


@pytest.mark.parametrize("mode", [0, 1], ids=["gbm", "xgb"])
@pytest.mark.parametrize("na_mass", [False, True], ids=["no_na", "na"])
@pytest.mark.parametrize("nvb_cat", [2, 37, 255])
@pytest.mark.parametrize("nbt", [64, 256])
def test_categorical_scan_matches_plain_loop(nbt, nvb_cat, na_mass, mode):
    """LevelScan's categorical rows (sorted with argsort and scattered back to
    bin ids) against plain_cat_best, a loop over the levels written on its own:
    gain, code, left totals and the row totals to the bit, and the left set.
    nvb 255 under nbt 64 is cut to the 63 scanned bins, as min(nvb[f], nbt - 1)
    says.  Both take the key as float64(G_int) / float64(S_int) and break ties
    on the bin id; neither looks at mono (the kernel's categorical scan applies
    no mono_ok: the scan with a sign on every feature gives the same rows)."""
    G, S, nvb = cat_level(nbt, nvb_cat, na_mass, 7 * nbt + nvb_cat + mode)
    ig, is_ = 2.0 ** -12, 2.0 ** -8
    p = TreeParams(mode=mode, min_rows=6.0, min_child_weight=6.0 if mode else 0.0, reg_lambda=1.0 if mode else 0.0,
                   reg_alpha=0.25 if mode else 0.0)
    allowed = np.ones((6, 3), bool)
    sc = Q.LevelScan(G, S, nvb, p, ig, is_, allowed, np.ones(3, bool))
    signed = Q.LevelScan(G, S, nvb, p, ig, is_, allowed, np.ones(3, bool), np.array([1, -1, 1]))
    assert np.array_equal(sc.gains, signed.gains) and np.array_equal(sc.f_code, signed.f_code)
    winners = 0
    for i in range(6):
        for f in range(3):
            want = plain_cat_best(G[i, f].tolist(), S[i, f].tolist(), int(nvb[f]), nbt, ig, is_, p)
            assert sc.f_G[i, f] == float(G[i, f].sum()) * ig and sc.f_S[i, f] == float(S[i, f].sum()) * is_
            if want is None:
                assert sc.f_gain[i, f] == -np.inf and sc.f_code[i, f] == 0x7FFFFFFF, (i, f)
                continue
            winners += 1
            got = (float(sc.f_gain[i, f]), int(sc.f_code[i, f]), float(sc.f_GL[i, f]), float(sc.f_SL[i, f]))
            assert got == want[:4], (i, f, got, want)
            assert np.nonzero(sc.left_set(i, f, want[1] >> 1))[0].tolist() == want[4], (i, f)
            assert Q.bitset(sc.left_set(i, f, want[1] >> 1))[(nbt - 1) >> 5] >> ((nbt - 1) & 31) == 0, "NA bin in the set"
    if nbt == 256 and nvb_cat == 255:
        assert Q.bitset(sc.left_set(3, 0, int(sc.f_code[3, 0]) >> 1))[7] == 0x7FFFFFFF, "word 7 not filled"
    # a single level: no candidate, or (with NA mass) that level against the NA rows alone
    lone = nvb > 1
    assert ((sc.f_code[4][lone] == 2) if na_mass else (sc.f_gain[4] == -np.inf)).all(), sc.f_code[4]
    assert winners >= (8 if nvb_cat > 2 else 4)
    if nvb_cat >= 37:
        # the planted equal keys are told apart by the bin id alone
        key = sc.cat_key[0][0]
        vals, cnt = np.unique(key[key < np.inf], return_counts=True)
        assert cnt.max() >= 3
    assert bool((sc.f_code[sc.f_gain > -np.inf] & 1).any()) == na_mass, "NA-left winners need NA mass, and use it"


# ---- constraints and categorical splits on integer inputs -------------------------

def _int_cat_case():
    """_int_data with column 0 replaced by 37 levels (3 % NaN) of shuffled effect
    and the 4-valued column 5 declared categorical"""
    if "cat" not in _int_cache:
        from h2omx.models.tree.binning import categorical_bins

        rng = np.random.default_rng(6)
        X, _ = _int_data()
        n = X.shape[1]
        lv = rng.integers(0, 37, n)
        eff = rng.permutation(37) / 6.0 - 3.0
        X[0] = lv
        X[0, rng.random(n) < 0.03] = np.nan
        sig = eff[lv] - 1.5 * X[1] * X[3] + 2.0 * np.nan_to_num(X[2], nan=-1.5) + 1.2 * X[5] - 1.8
        g = np.clip(np.rint(sig + rng.normal(size=n)), -8, 8).astype(np.float32)
        Xt = torch.from_numpy(X)
        e, nv, nbt = compute_edges(Xt, 63)
        e, nv, nbt, cat = categorical_bins(e, nv, nbt, {0: 37, 5: 4})
        _int_cache["cat"] = (bin_matrix(Xt, e, nv, nbt, cat=cat), g, cat)
    return _int_cache["cat"]


def _ref_and_oracle(bm, g, h, p, catf=None):
    n = bm.n
    ref = RefTreeBuilder(bm, p)
    ref.nid[:] = -1
    ref.nid[:n] = 0
    pad = np.zeros(bm.npad - n, np.float32)
    ones = np.ones(n, np.float32)
    want = ref.build(np.concatenate([g, pad]), np.concatenate([h, pad]), np.concatenate([ones, pad]), 0)
    info = {}
    got, leaf, records = Q.grow(bm.codes.numpy()[:, :n], bm.nvb.numpy(), bm.edges.numpy(), g, h, ones, p,
                                Q.unit_scales(), 0, 0, dither=False, catf=catf, info=info)
    keep = reachable(want)
    assert keep == reachable(got)
    assert np.array_equal(leaf, ~ref.nid[:n])
    return ref, want, got, keep, records, info


def _same_fields(want, got, keep, fields):
    for fld in fields:
        a, b = want[keep][fld], got[keep][fld]
        if fld == "thr":        # NaN marks a categorical split: the payload bits are nobody's contract
            assert np.array_equal(np.isnan(a), np.isnan(b))
            a, b = np.nan_to_num(a, nan=0.0), np.nan_to_num(b, nan=0.0)
        assert a.tobytes() == b.tobytes(), (fld, a, b)


_ALL_FIELDS = ("feat", "bin", "na_left", "left", "thr", "gain", "weight", "value")


@pytest.mark.parametrize("mode", [0, 1], ids=["gbm", "xgb"])
def test_categorical_trees_match_reference_builder(mode):
    """integer g, h = w = 1, unit scales, no dither: categorical set splits of
    both builders agree field by field, bitset by bitset and row by row.  The
    reference orders float64 histogram sums, the oracle int64 ones; on integer
    inputs the keys are the same quotients."""
    bm, g, cat = _int_cat_case()
    p = TreeParams(max_depth=5, min_rows=10, min_child_weight=10.0 if mode else 0.0, mode=mode,
                   reg_lambda=1.0 if mode else 0.0)
    ref, want, got, keep, records, info = _ref_and_oracle(bm, g, np.ones(bm.n, np.float32), p, cat)
    _same_fields(want, got, keep, _ALL_FIELDS)
    cats = [i for i in keep if want[i]["feat"] >= 0 and want[i]["na_left"] & 2]
    assert len(cats) >= 5 and {int(want[i]["feat"]) for i in cats} <= {0, 5}
    assert any(want[i]["na_left"] == 3 for i in cats), "no categorical split with NA left"
    assert np.array_equal(ref.catbits[cats], info["catbits"][cats])
    assert not info["catbits"][[i for i in keep if i not in cats]].any()
    assert any(want[i]["feat"] >= 0 and not want[i]["na_left"] & 2 for i in keep), "no numeric split"


@pytest.mark.parametrize("mode,hmax", [(0, 1), (0, 3), (1, 1), (1, 3)], ids=["gbm", "gbm_h", "xgb", "xgb_h"])
def test_monotone_trees_match_reference_builder(mode, hmax):
    """monotone (-1, +1, -1, 0, 0, +1, 0) on integer inputs (the gradients rise
    with columns 0, 2 and 5, so the values fall: the sign on column 5 goes
    against the data and bars its best splits), against the reference builder: the candidates
    mono_ok removes, the intervals and every clamped value.  Mode 0 has Newton
    leaves, so both builders re-derive the intervals
    from the subtree (G, H) sums (mono_newton_kernel / _mono_newton_refine);
    with integer h in 1 .. 3 those differ from the (G, W) the splits saw.
    Difference of the two definitions: the reference gives an INTERNAL node the
    value -G / H of its own sums and the weight W, the kernels (and the oracle)
    -G / S and S of the histogram's (S = W in mode 0, H in mode 1) - so with
    h != 1 the internal values (mode 0) and weights (mode 1) are compared only
    where the two coincide, on the leaves."""
    bm, g = _int_case(63)
    rng = np.random.default_rng(8)
    h = rng.integers(1, hmax + 1, bm.n).astype(np.float32)
    p = TreeParams(max_depth=5, min_rows=10, min_child_weight=10.0 if mode else 0.0, mode=mode,
                   reg_lambda=1.0 if mode else 0.0, learn_rate=0.5, monotone=(-1, 1, -1, 0, 0, 1, 0))
    ref, want, got, keep, records, info = _ref_and_oracle(bm, g, h, p)
    assert info["newton"] == (mode == 0)
    _same_fields(want, got, keep, _ALL_FIELDS[:-2])
    leaves = [i for i in keep if want[i]["feat"] < 0]
    inner = [i for i in keep if want[i]["feat"] >= 0]
    _same_fields(want, got, leaves if (mode == 0 and hmax > 1) else keep, ("value",))
    _same_fields(want, got, leaves if (mode == 1 and hmax > 1) else keep, ("weight",))
    # the constraints bit: against the unconstrained tree, and in the records
    free = Q.grow(bm.codes.numpy()[:, : bm.n], bm.nvb.numpy(), bm.edges.numpy(), g, h, np.ones(bm.n, np.float32),
                  TreeParams(**{**p.__dict__, "monotone": None}), Q.unit_scales(), 0, 0, dither=False)[0]
    assert free[: len(got)].tobytes() != got.tobytes()
    sp = [r for r in records if r["split"]]
    assert any((r["free_feat"], r["free_code"]) != (r["feat"], 2 * r["bin"] + r["na_left"]) for r in sp)
    assert any(r["cut"] for r in sp) and {int(want[i]["feat"]) for i in inner} >= {0, 2}
    final = 3 if mode == 0 else 2
    assert any(c[final] != c[1] for c in info["leaf_clamps"]), "no clamped leaf"
    # monotone along the constrained features: left subtree below / above right
    for i in inner:
        mf = p.monotone[int(want[i]["feat"])]
        if mf:
            def span(r):
                st, vals = [r], []
                while st:
                    j = st.pop()
                    if got[j]["feat"] < 0:
                        vals.append(float(got[j]["value"]))
                    else:
                        st += [int(got[j]["left"]), int(got[j]["left"]) + 1]
                return min(vals), max(vals)
            l, r = span(int(got[i]["left"])), span(int(got[i]["left"]) + 1)
            assert (l[1] <= r[0]) if mf > 0 else (l[0] >= r[1]), (i, l, r)


def test_monotone_on_a_categorical_feature_cuts_intervals_unchecked():
    """What the kernels do with a sign on a categorical column, pinned in the
    oracle as it stands in lf_write_node: the categorical scan applies no
    mono_ok, yet the children's intervals are cut by mono[feat] whatever the
    kind of the split.  The estimators reject such a constraint before it gets
    here (tests/test_monotone.py::test_monotone_validation); the reference
    builder, which does test mono on the sorted prefixes, is therefore not
    comparable on this input."""
    bm, g, cat = _int_cat_case()
    n = bm.n
    ones = np.ones(n, np.float32)
    args = (bm.codes.numpy()[:, :n], bm.nvb.numpy(), bm.edges.numpy(), g, ones, ones)
    p = TreeParams(max_depth=3, min_rows=10, mode=1, reg_lambda=1.0, monotone=(1, 0, 0, 0, 0, 0, 0))
    info = {}
    tree, _, records = Q.grow(*args, p, Q.unit_scales(), 0, 0, dither=False, catf=cat, info=info)
    free = Q.grow(*args, TreeParams(**{**p.__dict__, "monotone": None}), Q.unit_scales(), 0, 0, dither=False,
                  catf=cat)[0]
    node = records[1]
    assert node["gid"] == 1 and node["cat"] and node["feat"] == 0 and node["cut"]
    for fld in ("feat", "bin", "na_left", "left", "gain"):
        assert np.array_equal(tree[fld], free[fld]), fld        # the same splits as without the sign ...
    l = node["left"]
    assert info["lo"][l + 1] == info["hi"][l] and np.isfinite(info["hi"][l])     # ... under cut intervals


@pytest.mark.parametrize("inter", [((0, 1), (2, 3)), ((0, 1), (3, 5)), ((0, 1, 2), (2, 3))],
                         ids=["pairs", "root_unlisted", "overlap"])
def test_interaction_trees_match_reference_builder(inter):
    """interaction sets, the other features unlisted, on integer inputs: the
    oracle's istate against the reference builder's.  An unlisted feature can
    only be taken at the root (then the whole tree stays on it): the second
    case leaves the strongest column out of every set; the third shares column
    2 between its sets, so a split on it keeps both and a later one narrows."""
    bm, g = _int_case(63)
    p = TreeParams(max_depth=6, min_rows=10, interactions=inter)
    ref, want, got, keep, records, info = _ref_and_oracle(bm, g, np.ones(bm.n, np.float32), p)
    _same_fields(want, got, keep, _ALL_FIELDS)
    sp = [r for r in records if r["split"]]
    if inter == ((0, 1), (3, 5)):
        assert sp[0]["feat"] == 2 and all(r["feat"] == 2 and r["isolo"] == 2 for r in sp[1:]) and len(sp) > 5
    else:
        assert any(r["free_barred"] for r in sp)
        assert any(r["isolo"] == -1 and r["imask"] in (1, 2) for r in sp)
    if inter == ((0, 1, 2), (2, 3)):
        assert any(r["isolo"] == -1 and r["imask"] == 3 for r in sp), "no node below a split on the shared column"
    # every root path stays inside one set, or on one unlisted feature
    sets = [set(s) for s in inter] + [{f} for f in range(7) if not any(f in s for s in inter)]
    paths = {0: set()}
    for i in sorted(keep):
        if got[i]["feat"] >= 0:
            used = paths[i] | {int(got[i]["feat"])}
            assert any(used <= s for s in sets), (i, used)
            paths[int(got[i]["left"])] = paths[int(got[i]["left"]) + 1] = used


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

def cpu_boost(name, trees_out=None, infos_out=None):
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
            info = {}
            tree, leaf, rec = Q.grow(codes, nv, e, g, h, w, p, qs, 0, t * K + k, _tree_fmask(p, F, t, None),
                                     catf=case_catf(name), info=info)
            Fm[k] += tree["value"][leaf]
            counts.append(Q.near_tie_nodes(rec))
            if trees_out is not None:
                trees_out.append(tree)
            if infos_out is not None:
                infos_out.append(info)
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
    trees, infos = [], []
    counts = cpu_boost(name, trees, infos)
    print(name, "near-tie nodes per tree:", counts)
    assert max(counts) <= 1, counts
    # the audit is of real trees
    depth = CASES[name]["tp"]["max_depth"]
    assert all(len(t) > 4 * depth for t in trees), [len(t) for t in trees]
    if name in NEW_CASES:
        # no near-tie at all, and the case exercises what it is for
        assert max(counts) == 0, counts
        print(name, "witnesses:", case_witnesses(name, infos))
