"""The data sets and training configurations of the exact-oracle tests
(tests/test_quantref.py audits them on the CPU, tests/test_tree_oracle_gpu.py
trains them on the GPU and verifies every tree with tests/quantref.py)."""
import numpy as np

N = 20037       # not a multiple of 16 / 64 / 1024
N_PK32 = 600_000


def _mixed(n, F, seed, task):
    """continuous columns, one with 10 % NaN, one 4-valued"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(F, n)).astype(np.float32)
    X[2, rng.random(n) < 0.1] = np.nan
    X[5] = rng.integers(0, 4, n)
    logit = 1.5 * X[0] - X[1] * X[3] + np.nan_to_num(X[2]) + 0.7 * X[5]
    if task == "bin":
        y = (rng.random(n) < 1 / (1 + np.exp(-logit))).astype(np.float32)
    elif task == "reg":
        y = (logit + rng.normal(size=n)).astype(np.float32)
    elif task in ("count", "pos", "zpos"):
        mu = np.exp(np.clip(0.4 * logit, -3, 3))
        if task == "count":
            y = rng.poisson(mu).astype(np.float32)
        else:
            y = rng.gamma(2, mu / 2).astype(np.float32)
            if task == "zpos":
                y[rng.random(n) < 0.3] = 0.0
    elif task == "heavy":
        y = (logit + rng.standard_t(3, n)).astype(np.float32)
    else:
        y = np.digitize(logit, [-0.5, 1.5]).astype(np.float32)
    return X, y


def _cat(n, seed, big, task):
    """column 0: ``big`` levels of very unequal frequency whose effects have
    nothing to do with their codes, 3 % NaN (informative: it shifts the
    response); column 1: 5 levels; columns 2 .. 5 continuous"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(6, n)).astype(np.float32)
    pr = rng.dirichlet(np.full(big, 0.6))
    lv = rng.choice(big, n, p=pr)
    eff0, eff1 = rng.normal(size=big) * 1.3, np.array([0.9, -0.7, 0.2, -0.1, 0.5])
    small = rng.integers(0, 5, n)
    na = rng.random(n) < 0.03
    X[0], X[1] = lv, small
    X[0, na] = np.nan
    sig = np.where(na, 3.0, eff0[lv]) + eff1[small] + 0.8 * X[2] - 0.6 * X[3] * (small == 1) + 0.4 * np.abs(X[4])
    if task == "bin":
        y = (rng.random(n) < 1 / (1 + np.exp(-sig))).astype(np.float32)
    else:
        y = (sig + 0.5 * rng.normal(size=n)).astype(np.float32)
    return X, y


def _wiggly(n, seed, task):
    """the response rises with column 0 and falls with column 2 overall, but
    wiggles along both: unconstrained splits break the signs"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-3, 3, n), rng.normal(size=n), rng.uniform(0, 1, n), rng.normal(size=n),
                  rng.uniform(-1, 1, n)]).astype(np.float32)
    sig = X[0] + 1.5 * np.sin(3 * X[0]) + 0.5 * X[1] - 2.0 * X[2] + 0.8 * np.sin(9 * X[2]) + 0.6 * X[3] * X[4]
    if task == "bin":
        y = (rng.random(n) < 1 / (1 + np.exp(-sig))).astype(np.float32)
    else:
        y = (sig + 0.3 * rng.normal(size=n)).astype(np.float32)
    return X, y


def _pairs(n, seed, solo=1.4):
    """two interacting pairs (0, 1) and (2, 3), a feature 4 of strength ``solo``
    that belongs to no set (a root split on it leaves the whole tree nothing
    else), and a product across the pairs that the constraints forbid"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(5, n)).astype(np.float32)
    sig = 1.2 * X[0] * X[1] + X[0] + 1.0 * X[2] * X[3] + 0.8 * X[2] + solo * np.tanh(2 * X[4]) + 0.9 * X[1] * X[2]
    return X, (sig + 0.3 * rng.normal(size=n)).astype(np.float32)


def _fill256():
    from test_bundle_planes import _data_fill256

    X, y, _, _ = _data_fill256()
    return X, y


DATA = {
    "fill256": _fill256,       # NaNs, bundled 3-valued columns (tests/test_bundle_planes.py)
    "reg": lambda: _mixed(N, 7, 21, "reg"),
    "bin": lambda: _mixed(N, 7, 22, "bin"),
    "big": lambda: _mixed(N_PK32, 9, 23, "bin"),
    "multi": lambda: _mixed(N, 7, 24, "multi"),
    "drf": lambda: _mixed(N, 7, 25, "bin"),
    "count": lambda: _mixed(N, 7, 31, "count"),
    "pos": lambda: _mixed(N, 7, 32, "pos"),
    "zpos": lambda: _mixed(N, 7, 33, "zpos"),
    "heavy_laplace": lambda: _mixed(N, 7, 34, "heavy"),
    "heavy_quantile": lambda: _mixed(N, 7, 35, "heavy"),
    "heavy_huber": lambda: _mixed(N, 7, 36, "heavy"),
    "cat_reg": lambda: _cat(N, 41, 37, "reg"),
    "cat_bin": lambda: _cat(N, 42, 200, "bin"),
    "cat_drf": lambda: _cat(N, 43, 37, "bin"),
    "wiggly_reg": lambda: _wiggly(N, 44, "reg"),
    "wiggly_bin": lambda: _wiggly(N, 45, "bin"),
    "wiggly_xgb": lambda: _wiggly(N, 46, "reg"),
    "pairs": lambda: _pairs(N, 47),
    "pairs_deep": lambda: _pairs(N, 48, 0.6),
}

# name -> data set, nbins, train_ensemble arguments (wobs: seed of the observation
# weights, see case_weights), TreeParams arguments, engine ("scan" / "seg"),
# HipTreeBuilder class attributes to set
CASES = {
    "scan_defaults": dict(
        data="fill256", nbins=255, dist="bernoulli", ntrees=3, engine="scan",
        tp=dict(max_depth=5, min_rows=5, learn_rate=0.3), attrs={}),
    "scan_switches_off": dict(
        data="reg", nbins=63, dist="gaussian", ntrees=3, engine="scan",
        tp=dict(max_depth=6, min_rows=400, learn_rate=0.3),
        attrs=dict(FUSE_ROUTE=False, BUNDLE=False, FIN_PROLOGUE=False, PK32=False, L0_COPIES=1)),
    "xgb": dict(
        data="bin", nbins=255, dist="bernoulli", ntrees=3, engine="scan", sample_rate=0.7,
        tp=dict(max_depth=5, mode=1, reg_lambda=1.0, min_child_weight=1.0, gamma=0.0, learn_rate=0.3), attrs={}),
    "two_slot_passes": dict(
        data="fill256", nbins=255, dist="bernoulli", ntrees=2, engine="scan",
        tp=dict(max_depth=8, min_rows=5, learn_rate=0.3), attrs=dict(DEEP_LDS_BUDGET=64 * 1024)),
    "pk32": dict(
        data="big", nbins=255, dist="bernoulli", ntrees=2, engine="scan",
        tp=dict(max_depth=5, min_rows=10, learn_rate=0.3), attrs=dict(TARGET_WGS=8)),
    "multinomial": dict(
        data="multi", nbins=255, dist="multinomial", nclass=3, ntrees=2, engine="scan",
        tp=dict(max_depth=4, min_rows=10, learn_rate=0.3), attrs={}),
    "seg_drf": dict(
        data="drf", nbins=20, dist="drf", nclass=2, ntrees=3, engine="seg",
        sample_rate=0.632,
        tp=dict(max_depth=7, min_rows=5, learn_rate=1.0, leaf_mode=1, mtries=3), attrs=dict(BAG_COMPACT=True)),
}
for _name, _wave in (("seg_drf_direct_wg", 0), ("seg_drf_direct_wave", 1 << 30)):
    CASES[_name] = dict(CASES["seg_drf"],
                        attrs=dict(BAG_COMPACT=True, DIRECT_MIN_NODES=2, DIRECT_WAVE_ROWS=_wave))

# the gradient passes of the remaining distributions (tests/gradref.py closes the
# chain data -> gradients -> tree -> margins), with observation weights and a bag
_GRAD = dict(ntrees=3, engine="scan", attrs={})
CASES.update({
    "poisson_w": dict(_GRAD, data="count", nbins=63, dist="poisson", wobs=77,
                      tp=dict(max_depth=5, min_rows=10, learn_rate=0.3)),
    "gamma": dict(_GRAD, data="pos", nbins=255, dist="gamma", tp=dict(max_depth=4, min_rows=10, learn_rate=0.3)),
    "tweedie": dict(_GRAD, data="zpos", nbins=255, dist="tweedie", dist_kw=dict(tweedie_power=1.2),
                    tp=dict(max_depth=4, min_rows=10, learn_rate=0.3)),
    "laplace": dict(_GRAD, data="heavy_laplace", nbins=63, dist="laplace",
                    tp=dict(max_depth=5, min_rows=10, learn_rate=0.3)),
    "quantile_bag": dict(_GRAD, data="heavy_quantile", nbins=255, dist="quantile", dist_kw=dict(quantile_alpha=0.3),
                         sample_rate=0.7, tp=dict(max_depth=5, min_rows=10, learn_rate=0.3)),
    "huber_w": dict(_GRAD, data="heavy_huber", nbins=255, dist="huber", dist_kw=dict(huber_delta=0.8), wobs=77,
                    tp=dict(max_depth=5, min_rows=10, learn_rate=0.3)),
})

# categorical set splits, monotone and interaction constraints.  ``cat``: feature
# -> number of levels (binning.categorical_bins); TreeParams carries the
# constraints.  The witnesses each case is for are asserted from the oracle's
# records (case_witnesses), on the CPU audit and again on the GPU-built trees.
_MONO = (1, 0, -1, 0, 0)
CASES.update({
    "cat_gauss": dict(data="cat_reg", nbins=63, cat={0: 37, 1: 5}, dist="gaussian", ntrees=3, engine="scan",
                      tp=dict(max_depth=5, min_rows=10, learn_rate=0.3), attrs={}),
    "cat_bern_256": dict(data="cat_bin", nbins=255, cat={0: 200, 1: 5}, dist="bernoulli", ntrees=2, engine="scan",
                         sample_rate=0.7, tp=dict(max_depth=5, min_rows=10, learn_rate=0.3), attrs={}),
    "cat_seg_drf": dict(data="cat_drf", nbins=63, cat={0: 37, 1: 5}, dist="drf", nclass=2, ntrees=2, engine="seg",
                        sample_rate=0.632, tp=dict(max_depth=6, min_rows=5, learn_rate=1.0, leaf_mode=1, mtries=3),
                        attrs=dict(BAG_COMPACT=True, DIRECT_MIN_NODES=2)),
    "mono_sqerr": dict(data="wiggly_reg", nbins=63, dist="gaussian", ntrees=3, engine="scan",
                       tp=dict(max_depth=5, min_rows=10, learn_rate=0.3, monotone=_MONO), attrs={}),
    "mono_newton": dict(data="wiggly_bin", nbins=63, dist="bernoulli", ntrees=3, engine="scan",
                        tp=dict(max_depth=4, min_rows=10, learn_rate=0.3, mode=0, leaf_mode=0, monotone=_MONO),
                        attrs={}),
    "mono_xgb": dict(data="wiggly_xgb", nbins=255, dist="gaussian", ntrees=3, engine="scan",
                     tp=dict(max_depth=5, mode=1, reg_lambda=1.0, min_child_weight=1.0, gamma=0.0, learn_rate=0.3,
                             monotone=_MONO), attrs={}),
    "inter_scan": dict(data="pairs", nbins=63, dist="gaussian", ntrees=3, engine="scan",
                       tp=dict(max_depth=6, min_rows=10, learn_rate=0.3, interactions=((0, 1), (2, 3))), attrs={}),
    "inter_seg_deep": dict(data="pairs_deep", nbins=20, dist="gaussian", ntrees=2, engine="seg",
                           tp=dict(max_depth=12, min_rows=3, learn_rate=0.3, interactions=((0, 1), (2, 3))),
                           attrs={}),
})
NEW_CASES = ("cat_gauss", "cat_bern_256", "cat_seg_drf", "mono_sqerr", "mono_newton", "mono_xgb", "inter_scan",
             "inter_seg_deep")

_cache = {}


def case_data(name):
    """(X, y, edges, nvb, nbt, host codes [F][n]) of a case, computed once and left unchanged"""
    c = CASES[name]
    key = (c["data"], c["nbins"], tuple(sorted(c.get("cat", {}).items())))
    if key not in _cache:
        import torch

        from h2omx.models.tree import bin_matrix, compute_edges
        from h2omx.models.tree.binning import categorical_bins

        X, y = DATA[c["data"]]()
        Xt = torch.from_numpy(X)
        e, nv, nbt = compute_edges(Xt, c["nbins"])
        cat = None
        if c.get("cat"):
            e, nv, nbt, cat = categorical_bins(e, nv, nbt, c["cat"])
            assert cat.sum() == len(c["cat"])
            cat.setflags(write=False)
        codes = bin_matrix(Xt, e, nv, nbt, cat=cat).codes.numpy()[:, : X.shape[1]].copy()
        for a in (X, y, e, nv, codes):
            a.setflags(write=False)
        _cache[key] = (X, y, e, nv, nbt, codes, cat)
    return _cache[key][:6]


def case_catf(name):
    """bool [F] categorical flags of a case (binning.categorical_bins), or None"""
    case_data(name)
    c = CASES[name]
    return _cache[(c["data"], c["nbins"], tuple(sorted(c.get("cat", {}).items())))][6]


def case_weights(name):
    """observation weights of a case (float32, uniform in [0.5, 2)), or None"""
    c = CASES[name]
    if "wobs" not in c:
        return None
    n = case_data(name)[0].shape[1]
    return np.random.default_rng(c["wobs"]).uniform(0.5, 2, n).astype(np.float32)


def tree_params(name):
    from h2omx.models.tree import TreeParams

    return TreeParams(seed=5, **CASES[name]["tp"])


def builder_class(name):
    """HipTreeBuilder with the case's class attributes (host-side planning without a device)"""
    from h2omx.models.tree.engine import HipTreeBuilder

    return type("CaseBuilder", (HipTreeBuilder,), dict(CASES[name]["attrs"]))


def cat_level(nbt, nvb_cat, na_mass, seed, numeric_row=False):
    """Histograms of our own for the categorical scan: six nodes x three
    categorical rows (nvb_cat, 2 and 5 levels) of random int64 (G, S), and on
    request a fourth, numeric row.  40 % empty levels, levels of equal key (the
    same (G, S), and (G, S) against (2G, 2S)), a level with S > 0 and G == 0,
    mass in the bins past nvb (totals only); node 3's levels 224 .. 254 (nvb 255
    under nbt 256) hold the lowest keys, so its left set fills bitset word 7;
    node 4 has a single non-empty level in every row (no candidate without NA
    mass), node 5 every level on one key.  Returns (G, S, nvb)."""
    rng = np.random.default_rng(seed)
    F = 4 if numeric_row else 3
    nvb = np.array([nvb_cat, 2, 5, nbt * 3 // 4][:F], np.int32)
    S = rng.integers(1, 3000, (6, F, nbt))
    S[rng.random(S.shape) < 0.4] = 0
    G = np.where(S > 0, rng.integers(-(1 << 18), 1 << 18, S.shape), 0)
    G[:, :, nbt - 1], S[:, :, nbt - 1] = (-70000, 2500) if na_mass else (0, 0)
    m = min(nvb_cat, nbt - 1)
    for node in range(4):
        if m >= 8:
            a, b, c, z = rng.choice(min(m, 200), 4, replace=False)
            S[node, 0, a] = S[node, 0, b] = 700
            G[node, 0, a] = G[node, 0, b] = 12345          # equal keys, equal sums
            S[node, 0, c], G[node, 0, c] = 1400, 24690      # the same key from other sums
            S[node, 0, z], G[node, 0, z] = 900, 0
        S[node, 1, :2], G[node, 1, :2] = (1800, 2900), (0, -5000)
    if m == 255:
        S[3, 0, 224:255] = 2000
        G[3, 0, 224:255] = -(1 << 30) + np.arange(31)
    S[4, :, : nbt - 1], G[4, :, : nbt - 1] = 0, 0
    S[4, :, 1], G[4, :, 1] = 5000, 777
    S[5, :, : nbt - 1] = np.where(S[5, :, : nbt - 1] > 0, 64 * (1 + np.arange(nbt - 1) % 3), 0)
    G[5] = -3 * S[5]
    G[5, :, nbt - 1], S[5, :, nbt - 1] = G[0, :, nbt - 1], S[0, :, nbt - 1]
    return G.astype(np.int64), S.astype(np.int64), nvb


# ---------------------------------------------------------------------------
# what each constrained case is for, read off the oracle's own records
# ---------------------------------------------------------------------------
def case_witnesses(name, infos):
    """Assert that the trees of a case exercise what the case exists for.
    ``infos``: one ``info`` dict of quantref.grow / quantref.verify per tree.
    Returns the witness counts (printed by the tests)."""
    recs = [r for info in infos for r in info["records"]]
    splits = [r for r in recs if r["split"]]
    seen = {}
    if name.startswith("cat_"):
        cats = [r for r in splits if r["cat"]]
        seen["categorical splits"] = len(cats)
        seen["left sets with a gap in code order"] = sum(
            1 for r in cats if len(r["left_levels"]) >= 2 and (np.diff(r["left_levels"]) > 1).any())
        seen["categorical splits with NA left"] = sum(1 for r in cats if r["na_left"] == 1)
        below = 0
        for info in infos:
            parent = {}
            by_gid = {r["gid"]: r for r in info["records"]}
            for r in info["records"]:
                if r["split"]:
                    parent[r["left"]] = parent[r["left"] + 1] = r["gid"]
            for r in info["records"]:
                if r["split"] and not r["cat"]:
                    g = r["gid"]
                    while g in parent:
                        g = parent[g]
                        if by_gid[g]["cat"]:
                            below += 1
                            break
        seen["numeric splits below a categorical one"] = below
        seen["left sets in more than one bitset word"] = sum(
            1 for r in cats if len({b >> 5 for b in r["left_levels"]}) > 1)
        seen["nodes with an empty level (S_int == 0)"] = sum(1 for r in cats if r["empty_levels"] > 0)
        assert seen["categorical splits"] > 0 and seen["left sets with a gap in code order"] > 0, seen
        if name == "cat_gauss":
            assert seen["categorical splits with NA left"] > 0 and seen["numeric splits below a categorical one"] > 0, seen
        if name == "cat_bern_256":
            assert seen["left sets in more than one bitset word"] > 0, seen
            assert seen["nodes with an empty level (S_int == 0)"] > 0, seen
    if name.startswith("mono_"):
        newton = {info["newton"] for info in infos}
        # squared-error splits with Newton leaves take the re-derivation, XGBoost mode does not
        assert newton == {name != "mono_xgb"}, newton
        seen["winners after the best candidate failed mono_ok"] = sum(
            1 for r in splits if (r["free_feat"], r["free_code"]) != (r["feat"], 2 * r["bin"] + r["na_left"]))
        seen["intervals cut"] = sum(1 for r in splits if r["cut"] and np.isfinite(sum(r["child_intervals"][1:3])))
        final = 3 if name != "mono_xgb" else 2
        clamps = [c for info in infos for c in info["leaf_clamps"]]
        seen["leaves clamped"] = sum(1 for c in clamps if c[final] != c[1])
        assert all(v > 0 for v in seen.values()), seen
        if name == "mono_newton":
            seen["leaves clamped by the re-derived interval only"] = sum(
                1 for c in clamps if c[3] != c[1] and c[2] == c[1])
            # a tree that fills its capacity: mono_newton_kernel's depth walk must
            # still reach the last pair of children (left + 1 == capacity - 1)
            seen["full trees"] = sum(1 for info in infos if info["total"] == info["cap"])
            assert seen["leaves clamped by the re-derived interval only"] > 0 and seen["full trees"] > 0, seen
    if name.startswith("inter_"):
        seen["nodes whose best feature inter_ok bars"] = sum(1 for r in splits if r["free_barred"])
        seen["splits on the solo path of the unlisted feature"] = sum(1 for r in splits if r["isolo"] >= 0)
        seen["splits under a narrowed set mask"] = sum(1 for r in splits if r["isolo"] == -1 and r["imask"] in (1, 2))
        # (the deep case keeps its unlisted feature weak, so that the trees grow past it)
        assert all(v > 0 for k, v in seen.items() if name == "inter_scan" or "solo" not in k), seen
        assert all(r["feat"] == r["isolo"] for r in splits if r["isolo"] >= 0)
    return seen
