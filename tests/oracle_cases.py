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

_cache = {}


def case_data(name):
    """(X, y, edges, nvb, nbt, host codes [F][n]) of a case, computed once and left unchanged"""
    c = CASES[name]
    key = (c["data"], c["nbins"])
    if key not in _cache:
        import torch

        from h2omx.models.tree import bin_matrix, compute_edges

        X, y = DATA[c["data"]]()
        Xt = torch.from_numpy(X)
        e, nv, nbt = compute_edges(Xt, c["nbins"])
        codes = bin_matrix(Xt, e, nv, nbt).codes.numpy()[:, : X.shape[1]].copy()
        for a in (X, y, e, nv, codes):
            a.setflags(write=False)
        _cache[key] = (X, y, e, nv, nbt, codes)
    return _cache[key]


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
