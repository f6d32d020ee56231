"""CPU tests of the TreeSHAP reference (tests/shapref.py): its division-free
leaf formula against the Shapley definition and against rational arithmetic,
its table decoding against the tree-walking oracle of tests/test_explain.py,
the conditions the synthetic tables promise, and ``explain._shap_numpy`` (the
production path of CPU frames) held to the reference on every table."""
from fractions import Fraction

import numpy as np
import pytest

import shapref as SR
from h2omx.explain import _bucket, _shap_numpy, tree_paths

TABLES = SR.table_ids()


def _ids(t):
    return f"m{t[0]}-{t[1]}-F{t[2]}"


def _z(rng, m, lo=0.0, hi=1.0):
    return rng.uniform(lo, hi, m).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("pattern", ["all", "none", "mixed"])
def test_leaf_phi_is_the_shapley_definition(pattern):
    rng = np.random.default_rng(["all", "none", "mixed"].index(pattern))
    for trial in range(24):
        m = 1 + trial % 10
        z = _z(rng, m)
        if trial % 3 == 1:
            z[rng.integers(m)] = 1.0
        if trial % 3 == 2:
            z[rng.integers(m)] = 0.0
            z[rng.integers(m)] = 1.0
        o = {"all": np.ones(m), "none": np.zeros(m), "mixed": (rng.random(m) < 0.6).astype(float)}[pattern]
        v = float(rng.normal())
        got, want = SR.leaf_phi(z, o, v), SR.brute(z, o, v)
        assert got.shape == (m,)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, err_msg=f"m={m} z={z} o={o}")


def test_leaf_phi_rows_are_independent():
    rng = np.random.default_rng(5)
    z = _z(rng, 7)
    o = (rng.random((7, 11)) < 0.7).astype(float)
    both = SR.leaf_phi(z, o, 1.5)
    for r in range(11):
        np.testing.assert_array_equal(both[:, r], SR.leaf_phi(z, o[:, r], 1.5))


@pytest.mark.parametrize("m", [1, 2, 8, 9, 16, 17, 24, 28, 32])
def test_leaf_additivity(m):
    rng = np.random.default_rng(m)
    for lo, hi in SR.REGIMES.values():
        z = _z(rng, m, lo, hi)
        o = (rng.random((m, 40)) < 0.93).astype(float)
        o[:, 0] = 1.0
        o[:, 1] = 0.0
        v = float(rng.normal())
        phi = SR.leaf_phi(z, o, v)
        np.testing.assert_allclose(phi.sum(0), SR.leaf_total(z, o, v), rtol=0, atol=1e-12)


@pytest.mark.parametrize("m", [24, 32])
def test_leaf_phi_against_rational_arithmetic(m):
    rng = np.random.default_rng(100 + m)
    z = _z(rng, m, 0.95, 1.0)
    for followed in (1.0, 0.93, 0.5):
        o = (rng.random(m) < followed).astype(float)
        v = float(np.float32(rng.normal()))
        got = SR.leaf_phi(z, o, v)
        want = SR.exact(z, o, v)
        scale = max(abs(float(q)) for q in want)
        assert scale > 0
        err = max(float(abs(q - Fraction(float(g)))) for q, g in zip(want, got))
        assert err <= 1e-12 * scale, (m, followed, err, scale)


def test_follow_rule_by_hand():
    """Every branch of the follow rule on cells whose answer is plain to read."""
    inf = np.inf
    sets = np.stack([SR.level_set([0, 31, 32, 255]), SR.level_set([3])])

    NA, CAT = 1 << 30, 1 << 29
    # {z, lo, hi}; a categorical element keeps its set's index in lo
    E = np.array([(0, 0.5, -inf, 1.0), (0, 0.5, 1.0, inf), (0, 0.5, -1.0, 1.0),
                  (0, 0.5, 0.0, 0.0), (0, 0.5, 0.0, 0.0), (0, 0.5, 1.0, 0.0)], np.float32)
    E[:, 0] = np.array([0, 0 | NA, 0, 1 | CAT, 1 | NA | CAT, 1 | CAT], np.int32).view(np.float32)
    #             x0:  1.0 (on hi / on lo)  -1.0 (on lo)  nan    2.0    0.5
    #             x1:  0     31     32     255    256    -1     3.7    nan    4
    X = np.array([[1.0, -1.0, np.nan, 2.0, 0.5, 0.0, 0.0, 0.0, 0.0],
                  [0.0, 31.0, 32.0, 255.0, 256.0, -1.0, 3.7, np.nan, 4.0]])
    o = SR.follows(X, E, sets).astype(int)
    assert o[0].tolist() == [1, 1, 0, 0, 1, 1, 1, 1, 1]           # x <= 1, NaN refused
    assert o[1].tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0]           # x > 1 (1.0 itself not), NaN accepted
    assert o[2].tolist() == [1, 0, 0, 0, 1, 1, 1, 1, 1]           # -1 < x <= 1
    assert o[3].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0]           # set 0, out of range and NaN refused
    assert o[4].tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 0]           # set 0, out of range and NaN accepted
    assert o[5].tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 0]           # set 1 = {3}: 3.7 is level 3


@pytest.mark.parametrize("table", TABLES, ids=_ids)
def test_tables_meet_their_conditions(table):
    bucket, regime, F = table
    t, ref, tot = SR.reference(*table)
    X, lv, el, sets = t["X"], t["lv"], t["el"], t["sets"]
    assert X.shape == (F, SR.N_ROWS) and X.dtype == np.float32 and el.dtype == np.float32
    assert _bucket(t["maxm"]) == bucket and t["maxm"] == max(SR.WIDTHS[bucket])
    assert sorted(set(lv[:, 1].tolist())) == [0, *SR.WIDTHS[bucket]] and 28 <= len(lv) <= 32
    f, na_ok, cat, z, lo, hi = SR.decode(el)
    for start, m, _, _ in lv:
        assert len(set(f[start: start + m].tolist())) == m                     # distinct features in a leaf
    a, b = SR.REGIMES[regime]
    free = (z != 0.0) & (z != 1.0)
    assert (z == 1.0).sum() >= 2 and (z == 0.0).sum() == 1 and ((z[free] >= a) & (z[free] <= b)).all()
    num = ~cat
    assert (num & np.isinf(lo) & np.isfinite(hi)).any() and (num & np.isfinite(lo) & np.isinf(hi)).any()
    assert (num & np.isfinite(lo) & np.isfinite(hi)).any()
    for kind in (num, cat, f == SR.NAN_FEATURE):
        assert (kind & na_ok).any() and (kind & ~na_ok).any()
    assert set(f[cat].tolist()) == {1, F - 1} and len(sets) == cat.sum()
    for st in sets:
        assert all((int(st[b // 32]) >> (b % 32)) & 1 for b in SR.BASE_LEVELS)
    assert 0.04 < np.isnan(X[SR.NAN_FEATURE]).mean() < 0.14
    for c in (1, F - 1):
        assert {255.0, 256.0, -1.0, np.float32(3.7)} <= set(X[c, :4].tolist())
    all_follow = pairs = misses = elems = 0
    for start, m, _, _ in lv:
        if m:
            o = SR.follows(X, el[start: start + m], sets)
            all_follow += int(o.all(0).sum())
            pairs += o.shape[1]
            misses += int((~o).sum())
            elems += o.size
    assert all_follow >= 0.05 * pairs, all_follow / pairs
    assert misses >= 0.05 * elems, misses / elems
    assert np.abs(ref).max() > 0.05
    np.testing.assert_allclose(ref.sum(0), tot, rtol=0, atol=1e-12 * len(lv))


@pytest.mark.parametrize("table", TABLES, ids=_ids)
def test_shap_numpy_against_the_reference(table):
    """The bound: one rounding of a middle coefficient of P is 2^-53 C(32, 16)
    = 7e-8 per unit leaf value at the widest path, and the division carries it
    down to the constant term; ten times that, on the scale of the largest
    contribution."""
    t, ref, _ = SR.reference(*table)
    X = t["X"].astype(np.float64)
    tol = 1e-6 * max(1.0, float(np.abs(ref).max()))
    got = _shap_numpy(X, t["lv"], t["el"], t["maxm"], t["sets"])
    print(_ids(table), "max |_shap_numpy - shapref| =", np.abs(got - ref).max(), "tol", tol)
    np.testing.assert_allclose(got, ref, rtol=0, atol=tol)
    one = _shap_numpy(X[:, :1].copy(), t["lv"], t["el"], t["maxm"], t["sets"])
    np.testing.assert_allclose(one, ref[:, :1], rtol=0, atol=tol)


def test_contributions_against_the_tree_walk():
    """Pins the table decoding: the reference over ``tree_paths`` of a trained
    model equals Shapley values of the cover-weighted conditional expectation
    computed by walking the trees.

    The table keeps z in float32 and the walk divides the node covers in
    float64, which alone differ by 6e-8 relative.  So the trained trees keep
    their splits, NA directions and leaf values but get covers whose ratios are
    multiples of 1/16: a product of up to four of them has 16 bits and is the
    same number in both."""
    from test_explain import _data, brute_shap

    from h2omx.frame import Frame
    from h2omx.models import H2OGradientBoostingEstimator

    df = _data()
    m = H2OGradientBoostingEstimator(ntrees=6, max_depth=4, seed=1).train(y="y", training_frame=Frame.from_pandas(df))
    trees = m.ens.trees[: m.ens.ntrees].copy()
    for tr in trees:
        tr["weight"][0] = 65536.0
        stack = [0]
        while stack:
            i = stack.pop()
            if tr[i]["feat"] < 0:
                continue
            left = int(tr[i]["left"])
            wl, wr = float(tr[left]["weight"]), float(tr[left + 1]["weight"])
            sixteenths = min(15, max(1, round(16 * wl / (wl + wr))))
            tr["weight"][left] = tr[i]["weight"] * sixteenths / 16
            tr["weight"][left + 1] = tr[i]["weight"] * (16 - sixteenths) / 16
            stack += [left, left + 1]
    lv, el, _, maxm, sets = tree_paths(trees)
    rows = [0, 17, 34, 123, 500]                                   # 0, 17 and 34 hold a NaN
    X = df[list("pqrs")].values.astype(np.float64)[rows]
    assert np.isnan(X).any() and maxm >= 3
    got = SR.contributions(X.T, lv, el, sets)
    assert np.abs(got).max() > 0.05
    for i, x in enumerate(X):
        want = brute_shap(trees, x, 4)
        print("row", rows[i], "max |shapref - tree walk| =", np.abs(got[:, i] - want).max())
        np.testing.assert_allclose(got[:, i], want, rtol=0, atol=1e-9)
