"""Partial dependence on CPU frames (the general frame-substitution path):
2-D pairs, weights, the NA cell, single rows, argument order, the unchanged
1-D default, REST and client keywords, rejected inputs.

Bounds.  Tables are compared through their sums.  With u = 2**-52, n rows and
R = max |r| over the responses, a float64 sum of n terms bounded by T differs
from the exact sum by at most n u T whatever its order, so
    |n mean - sum r| <= n u R            (``tol_s``)
    |sum r^2 computed - exact| <= n u R^2  (``tol_s2``).
The references are exact sums (math.fsum).  For the spread, var0 = s2 / n -
mean^2 moves by at most tol_s2 / n + 2 R tol_s / n + (tol_s / n)^2 plus 4 u R^2
for its own three roundings, and |sqrt a - sqrt b| <= sqrt |a - b| gives
    |sd - sd_ref| <= sqrt(dvar0 m / (m - 1)).
"""
import math
import socket

import numpy as np
import pandas as pd
import pytest
import torch

from h2omx.explain import NA_LABEL, _response, partial_dependence
from h2omx.frame import Frame
from h2omx.frame.frame import DKV, ENUM, Vec
from h2omx.models import H2OGradientBoostingEstimator

N, U = 3000, 2.0 ** -52
NUM = ["f0", "f1", "f2", "f3", "f4"]
LEVELS = ["a", "b", "c", "d", "e"]


def _data(seed=7):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, 5)).astype(np.float32)
    e = rng.integers(0, 5, N)
    y = X[:, 0] * X[:, 1] + X[:, 2] + 0.5 * X[:, 3] + 0.7 * (e == 2) - 0.4 * (e == 4) + 0.1 * rng.normal(size=N)
    X[::11, 0] = np.nan
    X[3::17, 2] = np.nan
    d = {c: X[:, j] for j, c in enumerate(NUM)}
    d["e"] = np.array(LEVELS, dtype=object)[e]
    d["y"] = y.astype(np.float32)
    d["label"] = np.where(y > np.median(y), "yes", "no").astype(object)
    d["cls"] = np.array(["lo", "mid", "hi"], dtype=object)[np.digitize(y, np.quantile(y, [0.33, 0.66]))]
    d["w"] = rng.integers(0, 4, N).astype(np.float32)
    d["ones"] = np.ones(N, np.float32)
    return d


@pytest.fixture(scope="module")
def data():
    return _data()


@pytest.fixture(scope="module")
def frame(data):
    return Frame.from_numpy(data)


@pytest.fixture(scope="module")
def models(frame):
    x = NUM + ["e"]
    kw = dict(ntrees=20, max_depth=5, seed=1)
    return {"reg": (H2OGradientBoostingEstimator(**kw).train(x=x, y="y", training_frame=frame), None),
            "bin": (H2OGradientBoostingEstimator(balance_classes=True, **kw).train(x=x, y="label",
                                                                                   training_frame=frame), None),
            "multi": (H2OGradientBoostingEstimator(**kw).train(x=x, y="cls", training_frame=frame), "mid")}


def _forced(frame, col, value):
    """``frame`` with ``col`` overwritten by ``value`` (None: NA)."""
    v = frame.vec(col)
    n = frame.nrows
    if v.vtype == ENUM:
        nv = Vec(col, torch.full((n,), -1 if value is None else int(value), dtype=torch.int32), ENUM, list(v.domain))
    else:
        nv = Vec(col, torch.full((n,), float("nan") if value is None else float(value), dtype=torch.float32), v.vtype)
    return Frame([nv if u.name == col else u for u in frame.vecs])


def _resp(m, fr, target):
    return _response(m, m.predict_raw(fr), target).double().numpy()


def _check_row(row, r, w=None):
    """One table row against the responses r of its cell (exact sums)."""
    w = np.ones_like(r) if w is None else w
    keep = w > 0
    n, m, sw = len(r), int(keep.sum()), math.fsum(w)
    R = float(np.abs(r).max())
    wmax = float(w.max())
    tol_s, tol_s2 = n * U * R * wmax, n * U * R * R * wmax
    s, s2 = math.fsum(w * r), math.fsum(w * r * r)
    assert abs(row["mean_response"] * sw - s) <= tol_s
    mean = s / sw
    var0 = s2 / sw - mean * mean
    dvar = (tol_s2 + 2 * R * tol_s) / sw + (tol_s / sw) ** 2 + 4 * U * R * R
    sd = math.sqrt(max(var0, 0.0) * m / (m - 1))
    bound = math.sqrt(dvar * m / (m - 1))
    assert abs(row["stddev_response"] - sd) <= bound
    assert abs(row["std_error_mean_response"] - sd / math.sqrt(m)) <= bound / math.sqrt(m)


@pytest.mark.parametrize("which", ["reg", "bin", "multi"])
def test_2d_table_equals_explicit_predictions(models, frame, which):
    m, target = models[which]
    ga, gb = [-1.0, 0.0, 1.5], [-0.5, 0.25, 0.5, 2.0]
    tabs = m.partial_dependence(frame, col_pairs_2dpdp=[("f1", "f3")], target=target,
                                user_splits={"f1": ga, "f3": gb})
    assert len(tabs) == 1                                   # pairs without cols: the pairs alone
    t = tabs[0]
    assert t["columns"] == ["f1", "f3"] and t["target"] == target and len(t["data"]) == 12
    i = 0
    for a in ga:                                            # the first column varies slowest
        for b in gb:
            row = t["data"][i]
            assert row["f1"] == a and row["f3"] == b
            _check_row(row, _resp(m, _forced(_forced(frame, "f1", a), "f3", b), target))
            i += 1


def test_cols_then_pairs_and_default_grids(models, frame):
    m, _ = models["reg"]
    tabs = m.partial_dependence(frame, cols=["f1"], nbins=4, col_pairs_2dpdp=[["e", "f3"]])
    assert [("column" in t, "columns" in t) for t in tabs] == [(True, False), (False, True)]
    one = m.partial_dependence(frame, cols=["f3"], nbins=4)[0]["data"]
    pair = tabs[1]["data"]
    assert len(pair) == 5 * 4
    assert [r["e"] for r in pair[::4]] == LEVELS and [r["f3"] for r in pair[:4]] == [r["f3"] for r in one]


def test_weights_equal_repeated_rows(models, frame, data):
    m, _ = models["reg"]
    grid = [-1.0, 0.0, 1.0]
    got = partial_dependence(m, frame, "f1", user_splits=grid, weight_column="w")["data"]
    w = data["w"].astype(np.float64)
    rep = frame.rows(torch.from_numpy(np.repeat(np.arange(N), w.astype(np.int64))))
    assert rep.nrows == int(w.sum()) and (w == 0).any()
    for row, g in zip(got, grid):
        r = _resp(m, _forced(frame, "f1", g), None)
        _check_row(row, r, w)
        # the repeated frame has the same sum(w r) / sum(w) and uncorrected variance
        rr = _resp(m, _forced(rep, "f1", g), None)
        mean_rep = math.fsum(rr) / len(rr)
        var_rep = math.fsum(rr * rr) / len(rr) - mean_rep ** 2
        R = float(np.abs(r).max())
        mk = int((w > 0).sum())
        assert abs(row["mean_response"] - mean_rep) <= N * U * R * 3 / w.sum() + 2 * U * R
        var_got = row["stddev_response"] ** 2 * (mk - 1) / mk
        assert abs(var_got - var_rep) <= (3 * N * U * R * R * 3) / w.sum() + 8 * U * R * R


def test_unit_weights_change_nothing(models, frame):
    for which in ("reg", "bin"):
        m, _ = models[which]
        assert partial_dependence(m, frame, "f2", nbins=5, weight_column="ones") == \
            partial_dependence(m, frame, "f2", nbins=5)


@pytest.mark.parametrize("col", ["f0", "e"])
def test_include_na_appends_one_row(models, frame, col):
    m, _ = models["reg"]
    base = partial_dependence(m, frame, col, nbins=4)["data"]
    got = partial_dependence(m, frame, col, nbins=4, include_na=True)["data"]
    assert len(got) == len(base) + 1 and got[:-1] == base
    label = got[-1][col]
    assert label == NA_LABEL if col == "e" else math.isnan(label)
    _check_row(got[-1], _resp(m, _forced(frame, col, None), None))
    pair = partial_dependence(m, frame, "e", nbins=3, col2="f0", include_na=True)["data"]
    assert len(pair) == (5 + 1) * (3 + 1)                   # in 2-D the NA cell joins both columns
    assert pair[-1]["e"] == NA_LABEL and math.isnan(pair[-1]["f0"])
    _check_row(pair[-1], _resp(m, _forced(_forced(frame, "e", None), "f0", None), None))


def test_row_index(models, frame):
    m, _ = models["bin"]
    grid = [-1.0, 0.0, 1.0]
    i = 11                                                   # f0 is NA in this row
    got = partial_dependence(m, frame, "f1", user_splits=grid, row_index=i, weight_column="w")
    one = partial_dependence(m, frame.rows(torch.tensor([i])), "f1", user_splits=grid)
    assert got == one
    assert all(r["stddev_response"] == 0.0 and r["std_error_mean_response"] == 0.0 for r in got["data"])
    assert len({r["mean_response"] for r in got["data"]}) > 1
    with pytest.raises(ValueError, match=f"row_index {N} is outside the frame of {N} rows"):
        partial_dependence(m, frame, "f1", row_index=N)


def _parent_loop(model, frame, col, nbins=20, target=None, user_splits=None):
    """The 1-D partial dependence loop as it stood before the new keywords."""
    frame = model.adapt_frame(frame)
    v = frame.vec(col)
    n = frame.nrows
    if v.vtype == ENUM:
        dom = list(model.feature_domains.get(col) or v.domain or [])
        grid = list(range(len(dom)))
        labels = dom
    else:
        if user_splits is not None:
            grid = [float(a) for a in user_splits]
        else:
            x = v.as_float()
            ok = ~torch.isnan(x)
            lo_v, hi_v = float(x[ok].min().float()), float(x[ok].max().float())
            grid = list(np.linspace(lo_v, hi_v, nbins)) if hi_v > lo_v else [lo_v]
        labels = grid
    rows = []
    for g in grid:
        if v.vtype == ENUM:
            nv = Vec(col, torch.full((n,), int(g), dtype=torch.int32, device=v.data.device), ENUM, list(dom))
        else:
            nv = Vec(col, torch.full((n,), float(g), dtype=torch.float32, device=v.data.device), v.vtype)
        fr = Frame([nv if u.name == col else u for u in frame.vecs])
        r = _response(model, model.predict_raw(fr), target).double()
        st = torch.stack([r.sum(), (r * r).sum(), torch.tensor(float(n), dtype=torch.float64, device=r.device)])
        s, s2, cnt = (float(a) for a in st)
        mean = s / max(cnt, 1.0)
        sd = math.sqrt(max(s2 / max(cnt, 1.0) - mean * mean, 0.0) * cnt / max(cnt - 1.0, 1.0))
        rows.append({col: labels[len(rows)], "mean_response": mean, "stddev_response": sd,
                     "std_error_mean_response": sd / math.sqrt(max(cnt, 1.0))})
    return {"column": col, "target": target, "data": rows}


@pytest.mark.parametrize("which", ["reg", "bin", "multi"])
def test_default_call_is_unchanged(models, frame, which):
    m, target = models[which]
    for col in ("f0", "f3", "e"):
        assert partial_dependence(m, frame, col, nbins=6, target=target) == _parent_loop(m, frame, col, 6, target)
    assert m.partial_dependence(frame, ["f2"], nbins=3, target=target)[0] == _parent_loop(m, frame, "f2", 3, target)


def test_user_splits_keep_the_arguments_order(models, frame):
    m, _ = models["reg"]
    grid = [0.5, -1.0, 0.5, 2.0]
    got = partial_dependence(m, frame, "f3", user_splits=grid)["data"]
    assert [r["f3"] for r in got] == grid and got[0] == got[2]
    want = {r["f3"]: r for r in partial_dependence(m, frame, "f3", user_splits=sorted(set(grid)))["data"]}
    assert all(r == want[r["f3"]] for r in got)
    assert got[1]["mean_response"] < got[0]["mean_response"] < got[3]["mean_response"]     # y rises with f3


def test_rejected_inputs_name_the_column(models, frame):
    m, _ = models["reg"]
    with pytest.raises(ValueError, match="'f1' twice"):
        m.partial_dependence(frame, col_pairs_2dpdp=[("f1", "f1")])
    with pytest.raises(ValueError, match="'nope' is not in the frame"):
        m.partial_dependence(frame, col_pairs_2dpdp=[("f1", "nope")])
    with pytest.raises(ValueError, match="'y' is the response"):
        m.partial_dependence(frame, cols=["y"])
    with pytest.raises(ValueError, match="weight column 'f1' is a partial dependence column"):
        m.partial_dependence(frame, cols=["f1"], weight_column="f1")
    with pytest.raises(ValueError, match="weight column 'missing' is not in the frame"):
        m.partial_dependence(frame, cols=["f1"], weight_column="missing")


# -- REST and client ------------------------------------------------------------
@pytest.fixture(scope="module")
def conn(data, tmp_path_factory):
    from h2omx.api.server import H2OApi, serve
    from h2omx.client import H2OConnection
    from h2omx.runtime.cluster import ClusterConfig, form_cluster

    p = tmp_path_factory.mktemp("pd") / "pd.csv"
    pd.DataFrame({k: data[k] for k in NUM + ["e", "y", "w"]}).to_csv(p, index=False)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    srv = serve(H2OApi(form_cluster(ClusterConfig(), device="cpu")), "127.0.0.1", port)
    c = H2OConnection(f"http://127.0.0.1:{port}")
    c.import_file(str(p), destination_frame="pd.hex")
    mid = c.train("gbm", "pd.hex", y="y", x=NUM + ["e"], ntrees=5, max_depth=3, seed=1)["model_id"]["name"]
    yield c, mid
    srv.shutdown()
    DKV.clear()


def _column(table, name):
    return table["data"][[c["name"] for c in table["columns"]].index(name)]


def test_rest_pair_with_missing_na(conn):
    c, mid = conn
    r = c.request("POST /3/PartialDependence/", {"model_id": mid, "frame_id": "pd.hex", "nbins": 3,
                                                 "col_pairs_2dpdp": [["e", "f1"]], "add_missing_na": True})
    c.wait_job(r["job"])
    tabs = c.request(f"GET /3/PartialDependence/{r['destination_key']['name']}")["partial_dependence_data"]
    assert len(tabs) == 1 and tabs[0]["name"] == "2D-PartialDependence: e and f1"
    assert [col["name"] for col in tabs[0]["columns"]] == ["e", "f1", "mean_response", "stddev_response",
                                                           "std_error_mean_response"]
    assert tabs[0]["rowcount"] == (5 + 1) * (3 + 1)
    assert _column(tabs[0], "e")[-1] == NA_LABEL and _column(tabs[0], "f1")[-1] == "NaN"
    assert all(isinstance(a, float) for a in _column(tabs[0], "mean_response"))


def test_client_keywords(conn):
    c, mid = conn
    tabs = c.partial_dependence(mid, "pd.hex", cols=["f3"], col_pairs_2dpdp=[("f1", "f3")], weight_column="w",
                                include_na=True, user_splits={"f3": [1.0, -1.0], "f1": [0.0]})
    assert [t["rowcount"] for t in tabs] == [3, 2 * 3]
    assert _column(tabs[0], "f3") == [1.0, -1.0, "NaN"] and _column(tabs[1], "f1")[:3] == [0.0, 0.0, 0.0]
    plain = c.partial_dependence(mid, "pd.hex", cols=["f3"], user_splits={"f3": [1.0, -1.0]})[0]
    assert _column(plain, "mean_response") != _column(tabs[0], "mean_response")[:2]      # the weights count
    byidx = c.request("POST /3/PartialDependence/", {"model_id": mid, "frame_id": "pd.hex", "cols": ["f3"],
                                                     "weight_column_index": 7, "add_missing_na": True,
                                                     "user_cols": ["f3"], "user_splits": [1.0, -1.0],
                                                     "num_user_splits": [2]})
    c.wait_job(byidx["job"])
    t = c.request(f"GET /3/PartialDependence/{byidx['destination_key']['name']}")["partial_dependence_data"][0]
    assert t["data"] == tabs[0]["data"]                       # column 7 of the frame is w
    one = c.partial_dependence(mid, "pd.hex", cols=["f3"], row_index=5, user_splits={"f3": [1.0, -1.0]})[0]
    assert _column(one, "stddev_response") == [0.0, 0.0]
