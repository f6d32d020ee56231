"""Friedman-Popescu H statistic, ``model.h(frame, variables)``, on the CPU:
the path-table partial dependence and H against a node-by-node recursion on
the tree records that never touches the path table, the ordering of
interacting and additive pairs, stumps, variables no tree uses, the shard
combination of the moment helpers, the error cases and the REST / client
round trip (tests/test_friedman_h_gpu.py runs the HIP kernel)."""
import math
import socket

import numpy as np
import pandas as pd
import pytest
import torch

from h2omx.api.server import H2OApi, serve
from h2omx.client import H2OConnection, H2OResponseError
from h2omx.explain import _h_leaf_table, _h_moments, _h_pd_numpy, _h_sums, friedman_h, tree_paths
from h2omx.frame import Frame
from h2omx.frame.frame import DKV
from h2omx.models import (H2OGeneralizedLinearEstimator, H2OGradientBoostingEstimator,
                          H2OXGBoostEstimator)
from h2omx.runtime.cluster import ClusterConfig, form_cluster

N, F, NTREES, DEPTH = 600, 5, 20, 4
NAMES = [f"f{i}" for i in range(F)]


def _xy(seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, F)).astype(np.float32)
    y = X[:, 0] * X[:, 1] + X[:, 2] + 0.5 * X[:, 3] + 0.1 * rng.normal(size=N)
    X[::11, 0] = np.nan
    return X, y


@pytest.fixture(scope="module")
def frame():
    X, y = _xy()
    return Frame.from_numpy(np.c_[X, y], names=NAMES + ["y"])


@pytest.fixture(scope="module", params=["gbm", "xgboost"])
def model(request, frame):
    cls = {"gbm": H2OGradientBoostingEstimator, "xgboost": H2OXGBoostEstimator}[request.param]
    return cls(ntrees=NTREES, max_depth=DEPTH, seed=1).train(y="y", training_frame=frame)


def _matrix(m, fr):
    fr = m.adapt_frame(fr)
    X = m._matrix(fr) if hasattr(m, "_matrix") else fr.feature_matrix(m.x)
    return X.double().numpy()


def recursion_pd(ens, X, S):
    """Partial dependence on the feature set S of rows X [F][n] by the weighted
    traversal of the node records, float64: a split on a feature of S is
    followed, any other averages its children by their ``weight``."""
    n = X.shape[1]

    def rec(tr, i):
        nd = tr[i]
        f = int(nd["feat"])
        if f < 0:
            return np.full(n, float(nd["value"]))
        left = int(nd["left"])
        a, b = rec(tr, left), rec(tr, left + 1)
        if f in S:
            x = X[f]
            with np.errstate(invalid="ignore"):
                go_left = np.where(np.isnan(x), bool(int(nd["na_left"]) & 1), x <= float(nd["thr"]))
            return np.where(go_left, a, b)
        wl, wr = float(tr[left]["weight"]), float(tr[left + 1]["weight"])
        return (wl * a + wr * b) / float(nd["weight"])

    return sum(rec(ens.trees[t], 0) for t in range(ens.ntrees))


def recursion_h(ens, X, idx):
    k = len(idx)
    comb = np.zeros(X.shape[1])
    full = None
    for s in range(1, 1 << k):
        S = {idx[j] for j in range(k) if (s >> j) & 1}
        Fs = recursion_pd(ens, X, S)
        Fs = Fs - Fs.mean()
        comb += (-1.0) ** (k - len(S)) * Fs
        full = Fs
    num, den = float((comb * comb).sum()), float((full * full).sum())
    return math.sqrt(num / den) if num < den else float("nan")


def _table(m, idx):
    nt = m.ens.ntrees
    lv, el, _, maxm, _ = tree_paths(m.ens.trees[:nt], 1.0 / nt if m.ens.average else 1.0)
    return _h_leaf_table(lv, el, idx), maxm


def test_pathtable_pd_matches_recursion(model, frame):
    X = _matrix(model, frame)[:, :40]
    assert np.isnan(X[0]).any()
    vmax = max(float(np.abs(tr["value"][tr["feat"] < 0]).max()) for tr in model.ens.trees[:model.ens.ntrees])
    # every z of the table is one float32 rounding (2^-24 relative) and a leaf multiplies at most
    # maxm <= DEPTH of them
    tol = 4 * DEPTH * 2.0 ** -24 * NTREES * vmax
    for idx in ([0, 1], [2], [0, 1, 2]):
        if len(idx) == 1:                       # a single variable: the row of {2} in a 2-variable table
            table, maxm = _table(model, [idx[0], 4])
            got = _h_pd_numpy(X, table)[0]
        else:
            table, maxm = _table(model, idx)
            got = _h_pd_numpy(X, table)[-1]
        assert maxm <= DEPTH
        want = recursion_pd(model.ens, X, set(idx))
        print(idx, "max |path table - recursion| =", np.abs(got - want).max(), "tol", tol)
        np.testing.assert_allclose(got, want, rtol=0, atol=tol)


# measured on the CPU over both models and the three tuples below: the largest
# |H_pathtable - H_recursion| is 3.0e-9 (the float32 z of the table); 10x that
H_ORACLE_TOL = 3.0e-8


def test_h_matches_recursion_h(model, frame):
    X = _matrix(model, frame)
    for idx in ([0, 1], [2, 3], [0, 1, 2]):
        got = model.h(frame, [NAMES[i] for i in idx])
        want = recursion_h(model.ens, X, idx)
        print(model.algo, idx, "h", got, "recursion", want, "diff", abs(got - want))
        assert isinstance(got, float) and 0.0 < got < 1.0
        assert abs(got - want) <= H_ORACLE_TOL


def test_interacting_pair_ranks_first(model, frame):
    h01 = model.h(frame, ["f0", "f1"])
    others = [model.h(frame, v) for v in (["f2", "f3"], ["f0", "f2"], ["f1", "f4"])]
    print(model.algo, h01, others)
    assert all(h01 > o for o in others)
    assert model.h(frame, ["f1", "f0"]) == pytest.approx(h01, rel=1e-12)


def test_stumps_do_not_interact(frame):
    # the response has no main effect of f0 or f1: stumps reach them only after f2 and f3 are fitted
    m = H2OGradientBoostingEstimator(ntrees=120, max_depth=1, seed=1).train(y="y", training_frame=frame)
    used = {int(tr["feat"][0]) for tr in m.ens.trees[:m.ens.ntrees]}
    assert {0, 1, 2, 3} <= used
    for v in (["f0", "f1"], ["f2", "f3"], ["f0", "f1", "f2"]):
        h = m.h(frame, v)
        print("stumps", v, h)
        assert h < 1e-6                          # float64 sums give ~1e-16; float32 accumulation does not


def test_variable_no_tree_uses():
    X, y = _xy(3)
    X[:, 3] = 1.5
    X[:, 4] = -2.0
    fr = Frame.from_numpy(np.c_[X, y], names=NAMES + ["y"])
    m = H2OGradientBoostingEstimator(ntrees=10, max_depth=3, seed=1).train(y="y", training_frame=fr)
    used = {int(f) for tr in m.ens.trees[:m.ens.ntrees] for f in tr["feat"] if f >= 0}
    assert 0 in used and not used & {3, 4}
    assert m.h(fr, ["f0", "f3"]) == 0.0
    assert m.h(fr, ["f3", "f0"]) == 0.0
    assert math.isnan(m.h(fr, ["f3", "f4"]))


def test_moment_helpers_combine_over_shards(model, frame):
    X = _matrix(model, frame)
    for idx in ([0, 1], [0, 1, 2]):
        table, _ = _table(model, idx)
        A = torch.from_numpy(_h_pd_numpy(X[:, :250], table, const=False))
        B = torch.from_numpy(_h_pd_numpy(X[:, 250:], table, const=False))
        sums = _h_sums(A) + _h_sums(B)
        assert sums.shape == (2 ** len(idx),) and float(sums[-1]) == N
        means = sums[:-1] / sums[-1]
        num, den = (float(a) for a in _h_moments(A, means) + _h_moments(B, means))
        assert math.sqrt(num / den) == pytest.approx(model.h(frame, [NAMES[i] for i in idx]), rel=1e-12)


def test_error_cases(model, frame):
    with pytest.raises(ValueError, match="at least 2"):
        model.h(frame, ["f0"])
    with pytest.raises(ValueError, match="'f1'.*twice"):
        model.h(frame, ["f0", "f1", "f1"])
    with pytest.raises(ValueError, match="'nope'"):
        model.h(frame, ["f0", "nope"])
    rng = np.random.default_rng(5)
    wide = pd.DataFrame(rng.normal(size=(200, 11)), columns=[f"c{i}" for i in range(11)])
    wide["g"] = pd.Categorical(rng.choice(["u", "v", "w"], 200))
    wide["y"] = wide.c0 * wide.c1 + rng.normal(size=200)
    wfr = Frame.from_pandas(wide)
    m = H2OGradientBoostingEstimator(ntrees=2, max_depth=2, seed=1).train(y="y", training_frame=wfr)
    with pytest.raises(ValueError, match="'g'.*categorical"):
        m.h(wfr, ["c0", "g"])
    with pytest.raises(ValueError, match="at most 10.*'c10'"):
        m.h(wfr, [f"c{i}" for i in range(11)])
    assert isinstance(m.h(wfr, [f"c{i}" for i in range(10)]), float)
    multi = H2OGradientBoostingEstimator(ntrees=2, max_depth=2, seed=1).train(
        x=["c0", "c1"], y="g", training_frame=wfr)
    with pytest.raises(NotImplementedError):
        multi.h(wfr, ["c0", "c1"])
    glm = H2OGeneralizedLinearEstimator(family="gaussian", lambda_=0.0).train(
        x=["c0", "c1"], y="y", training_frame=wfr)
    with pytest.raises(NotImplementedError, match="glm"):
        glm.h(wfr, ["c0", "c1"])
    with pytest.raises(NotImplementedError):
        friedman_h(glm, wfr, ["c0", "c1"])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture()
def rest():
    api = H2OApi(form_cluster(ClusterConfig(), device="cpu"))
    srv = serve(api, "127.0.0.1", _free_port())
    yield api, H2OConnection(f"http://127.0.0.1:{srv.server_address[1]}")
    srv.shutdown()
    DKV.clear()


def test_rest_and_client_round_trip(rest):
    api, conn = rest
    X, y = _xy(7)
    df = pd.DataFrame(X, columns=NAMES)
    df["g"] = pd.Categorical(np.where(X[:, 4] > 0, "p", "q"))
    df["y"] = y
    DKV.put("fr.hex", Frame.from_pandas(df, key="fr.hex"))
    mid = conn.train("gbm", "fr.hex", y="y", ntrees=5, max_depth=3, seed=1)["model_id"]["name"]
    model = DKV.get(mid)
    want = model.h(DKV.get("fr.hex"), ["f0", "f1"])
    assert 0.0 < want < 1.0
    assert conn.h(mid, "fr.hex", ["f0", "f1"]) == pytest.approx(want, rel=1e-12)
    # handle() itself: a list, H2O's string form, and the error answers
    for variables in (["f0", "f1"], '["f0","f1"]'):
        status, _, out = api.handle("POST", "/3/FriedmansPopescusH",
                                    {"model_id": mid, "frame": "fr.hex", "variables": variables})
        assert status == 200 and out["__meta"]["schema_name"] == "FriedmanPopescusHV3"
        assert out["h"] == pytest.approx(want, rel=1e-12) and out["variables"] == ["f0", "f1"]
    status, _, err = api.handle("POST", "/3/FriedmansPopescusH",
                                {"model_id": mid, "frame": "nope.hex", "variables": ["f0", "f1"]})
    assert status == 404
    status, _, err = api.handle("POST", "/3/FriedmansPopescusH",
                                {"model_id": mid, "frame": "fr.hex", "variables": ["f0", "g"]})
    assert status >= 400 and "'g'" in err["msg"]
    with pytest.raises(H2OResponseError):
        conn.h(mid, "fr.hex", ["f0", "g"])
    with pytest.raises(H2OResponseError):
        conn.h(mid, "fr.hex", ["f0"])
