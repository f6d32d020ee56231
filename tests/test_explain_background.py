"""Interventional (baseline) SHAP, ``predict_contributions(frame,
background_frame=...)``, on the CPU: against a brute-force Shapley oracle that
enumerates every coalition of the hybrid-row game and never touches the path
table, additivity, the two output modes, the unchanged default form, the
error cases, the GLM form and the REST / client round trip
(tests/test_explain_background_gpu.py runs the HIP kernel)."""
import itertools
import math
import socket

import numpy as np
import pandas as pd
import pytest
import torch

from h2omx.api.server import H2OApi, serve
from h2omx.client import H2OConnection, H2OResponseError
from h2omx.explain import _shap_numpy, predict_contributions, tree_paths
from h2omx.frame import Frame
from h2omx.frame.frame import DKV
from h2omx.models import (H2OGeneralizedLinearEstimator, H2OGradientBoostingEstimator,
                          H2ORandomForestEstimator)
from h2omx.runtime.cluster import ClusterConfig, form_cluster


def _matrix(m, fr):
    fr = m.adapt_frame(fr)
    return m._matrix(fr) if hasattr(m, "_matrix") else fr.feature_matrix(m.x)


def brute_baseline_shap(m, X, B):
    """phi [n][nb][F] and margins of X and B: Shapley values of the game
    v(T) = margin(features T from x, the rest from b), every coalition scored
    by the model itself."""
    F, n = X.shape
    nb = B.shape[1]
    masks = list(itertools.product((False, True), repeat=F))
    rows = []
    for r in range(n):
        for b in range(nb):
            for T in masks:
                rows.append(torch.where(torch.tensor(T), X[:, r], B[:, b]))
    v = m.ens.raw_margin(torch.stack(rows, 1))[0].double().numpy().reshape(n, nb, len(masks))
    idx = {T: i for i, T in enumerate(masks)}
    phi = np.zeros((n, nb, F))
    for j in range(F):
        for T in masks:
            if T[j]:
                continue
            k = sum(T)
            w = math.factorial(k) * math.factorial(F - k - 1) / math.factorial(F)
            Tj = tuple(True if i == j else t for i, t in enumerate(T))
            phi[:, :, j] += w * (v[:, :, idx[Tj]] - v[:, :, idx[T]])
    return phi, m.ens.raw_margin(X)[0].double().numpy(), m.ens.raw_margin(B)[0].double().numpy()


def _data(n=3000, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 4)).astype(np.float32)
    X[::17, 1] = np.nan
    X[5::29, 3] = np.nan
    logit = X[:, 0] - np.nan_to_num(X[:, 1]) * X[:, 2] + 0.3 * np.nan_to_num(X[:, 3])
    y = np.where(rng.random(n) < 1 / (1 + np.exp(-logit)), "a", "b")
    df = pd.DataFrame(X, columns=list("pqrs"))
    df["y"] = pd.Categorical(y)
    return df


@pytest.fixture(scope="module")
def data():
    df = _data()
    fr = Frame.from_pandas(df)
    # scored rows 0 (q NA), 5 (s NA), 123; background rows 17 / 34 (q NA), 63 (s NA), 200, 301
    x = Frame.from_pandas(df.iloc[[0, 5, 123]].reset_index(drop=True))
    b = Frame.from_pandas(df.iloc[[17, 34, 63, 200, 301]].reset_index(drop=True))
    assert df.iloc[[0, 5]].isna().any(axis=1).all() and df.iloc[[17, 34, 63]].isna().any(axis=1).all()
    return fr, x, b


@pytest.fixture(scope="module", params=["gbm", "drf"])
def model(request, data):
    cls, kw = {"gbm": (H2OGradientBoostingEstimator, dict(ntrees=6, max_depth=3)),
               "drf": (H2ORandomForestEstimator, dict(ntrees=4, max_depth=4))}[request.param]
    return cls(seed=1, **kw).train(y="y", training_frame=data[0])


def test_background_shap_matches_bruteforce(model, data):
    _, x, b = data
    phi, mx, mb = brute_baseline_shap(model, _matrix(model, x), _matrix(model, b))
    avg = predict_contributions(model, x, background_frame=b).to_pandas()
    assert list(avg.columns) == ["p", "q", "r", "s", "BiasTerm"] and len(avg) == 3
    np.testing.assert_allclose(avg.values[:, :4], phi.mean(1), atol=1e-4)
    np.testing.assert_allclose(avg["BiasTerm"].values, np.full(3, mb.mean()), atol=1e-4)
    per = predict_contributions(model, x, background_frame=b, output_per_reference=True).to_pandas()
    assert list(per.columns) == ["RowIdx", "BackgroundRowIdx", "p", "q", "r", "s", "BiasTerm"] and len(per) == 15
    np.testing.assert_allclose(per.values[:, 2:6], phi.reshape(15, 4), atol=1e-4)
    np.testing.assert_allclose(per["BiasTerm"].values, np.tile(mb, 3), atol=1e-4)


def _cat_data(n=4000, nlev=20, seed=9):
    rng = np.random.default_rng(seed)
    levels = [f"L{i:02d}" for i in range(nlev)]
    hi = {lv for i, lv in enumerate(levels) if (i * 7) % 3 == 0}
    g = rng.choice(levels, n).astype(object)
    x = rng.normal(size=n)
    f = np.array([2.5 if v in hi else -0.5 for v in g]) + 0.4 * x
    g[rng.uniform(size=n) < 0.05] = None
    f = np.where(pd.isna(g), 4.0, f)
    return pd.DataFrame({"g": pd.Categorical(g, categories=levels), "x": x, "y": f + 0.1 * rng.normal(size=n)})


def test_background_shap_with_categorical_group_splits():
    df = _cat_data()
    m = H2OGradientBoostingEstimator(ntrees=6, max_depth=3, seed=1).train(
        x=["g", "x"], y="y", training_frame=Frame.from_pandas(df))
    assert m.ens.catbits is not None and any((int(tr[0]["na_left"]) & 2) for tr in m.ens.trees)
    x = Frame.from_pandas(pd.DataFrame({"g": pd.Categorical(["L00", "L01", None, "L07"]),
                                        "x": [0.3, -1.0, 0.5, np.nan]}))
    # background: a level unseen in training ("ZZZ" scores in the NA direction), an NA and seen levels
    b = Frame.from_pandas(pd.DataFrame({"g": pd.Categorical(["ZZZ", "L03", None, "L12", "L00"]),
                                        "x": [0.0, 1.5, -0.7, np.nan, 0.3]}))
    phi, mx, mb = brute_baseline_shap(m, _matrix(m, x), _matrix(m, b))
    per = predict_contributions(m, x, background_frame=b, output_per_reference=True).to_pandas()
    np.testing.assert_allclose(per[["g", "x"]].values, phi.reshape(20, 2), atol=1e-4)
    avg = predict_contributions(m, x, background_frame=b).to_pandas()
    np.testing.assert_allclose(avg[["g", "x"]].values, phi.mean(1), atol=1e-4)
    np.testing.assert_allclose(avg.values.sum(1), mx, atol=2e-4)


def test_additivity_and_self_reference(model, data):
    fr, _, _ = data
    x = fr.rows(torch.arange(0, 200))
    b = fr.rows(torch.arange(150, 190))            # overlaps the scored rows: pairs (r, r) exist
    mx = model.ens.raw_margin(_matrix(model, x))[0].numpy()
    mb = model.ens.raw_margin(_matrix(model, b))[0].numpy()
    avg = predict_contributions(model, x, background_frame=b).to_pandas()
    np.testing.assert_allclose(avg.values.sum(1), mx, atol=2e-4)
    np.testing.assert_allclose(avg["BiasTerm"].values, np.full(200, mb.mean()), atol=2e-4)
    per = predict_contributions(model, x, background_frame=b, output_per_reference=True).to_pandas()
    phi = per.values[:, 2:-1].reshape(200, 40, 4)
    np.testing.assert_allclose(per.values[:, 2:].sum(1), np.repeat(mx, 40), atol=2e-4)
    np.testing.assert_allclose(phi.sum(2), mx[:, None] - mb[None, :], atol=2e-4)
    np.testing.assert_allclose(per["BiasTerm"].values, np.tile(mb, 200), atol=2e-4)
    for r in range(150, 190):                       # a row explained against itself
        assert np.all(phi[r, r - 150] == 0.0)


def test_modes_agree_and_pairs_are_x_major(model, data):
    fr, _, _ = data
    x, b = fr.rows(torch.arange(40, 77)), fr.rows(torch.arange(300, 311))
    avg = predict_contributions(model, x, background_frame=b).to_pandas()
    per = predict_contributions(model, x, background_frame=b, output_per_reference=True).to_pandas()
    np.testing.assert_array_equal(per["RowIdx"].values, np.repeat(np.arange(37), 11))
    np.testing.assert_array_equal(per["BackgroundRowIdx"].values, np.tile(np.arange(11), 37))
    mean = per.groupby("RowIdx").mean().drop(columns="BackgroundRowIdx")
    assert list(mean.columns) == list(avg.columns)
    np.testing.assert_allclose(mean.values, avg.values, atol=1e-6)


def test_default_form_is_unchanged(model, data):
    fr = data[0]
    a = predict_contributions(model, fr)
    b = predict_contributions(model, fr, background_frame=None)
    c = model.predict_contributions(fr, background_frame=None, output_per_reference=False)
    assert a.names == b.names == c.names
    for u, v, w in zip(a.vecs, b.vecs, c.vecs):
        assert torch.equal(u.data, v.data) and torch.equal(u.data, w.data)
    # and it is still the path-dependent form of the path table
    nt = model.ens.ntrees
    lv, el, _, maxm, sets = tree_paths(model.ens.trees[:nt], 1.0 / nt if model.ens.average else 1.0)
    ref = _shap_numpy(_matrix(model, fr).double().numpy()[:, :50], lv, el, maxm, sets)
    got = torch.stack([v.data for v in a.vecs[:4]]).numpy()[:, :50]
    np.testing.assert_array_equal(got, ref.astype(np.float32))


def test_error_cases(model, data, monkeypatch):
    fr, x, b = data
    with pytest.raises(ValueError, match="background_frame"):
        predict_contributions(model, x, output_per_reference=True)
    with pytest.raises(ValueError, match="no rows"):
        predict_contributions(model, x, background_frame=b.rows(torch.arange(0)))
    with pytest.raises(TypeError):
        predict_contributions(model, x, b)          # keyword-only
    import h2omx.explain as ex

    monkeypatch.setattr(ex, "_CPU_CONTRIB_LIMIT", 100)
    with pytest.raises(ValueError, match=r"3 rows against 5 background rows.*420 bytes.*100 bytes"):
        predict_contributions(model, x, background_frame=b, output_per_reference=True)


def test_glm_background_contributions():
    rng = np.random.default_rng(3)
    n = 500
    df = pd.DataFrame({"u": rng.normal(2.0, 3.0, n), "w": rng.normal(-1.0, 0.5, n)})
    df["y"] = 1.5 * df.u - 2.0 * df.w + 0.7 + 0.01 * rng.normal(size=n)
    fr = Frame.from_pandas(df)
    glm = H2OGeneralizedLinearEstimator(family="gaussian", lambda_=0.0).train(y="y", training_frame=fr)
    coef = glm.coef()
    x, b = fr.rows(torch.arange(0, 7)), fr.rows(torch.arange(100, 104))
    xv, bv = df.iloc[:7], df.iloc[100:104]
    eta = lambda d: coef["Intercept"] + coef["u"] * d.u.values + coef["w"] * d.w.values   # noqa: E731
    per = glm.predict_contributions(x, background_frame=b, output_per_reference=True).to_pandas()
    assert list(per.columns) == ["RowIdx", "BackgroundRowIdx", "u", "w", "BiasTerm"] and len(per) == 28
    for c in ("u", "w"):
        ref = coef[c] * (xv[c].values[:, None] - bv[c].values[None, :])
        np.testing.assert_allclose(per[c].values.reshape(7, 4), ref, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(per["BiasTerm"].values, np.tile(eta(bv), 7), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(per[["u", "w", "BiasTerm"]].values.sum(1), np.repeat(eta(xv), 4), rtol=1e-5, atol=1e-5)
    avg = glm.predict_contributions(x, background_frame=b).to_pandas()
    assert list(avg.columns) == ["u", "w", "BiasTerm"]
    np.testing.assert_allclose(avg.values.sum(1), eta(xv), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(avg["u"].values, coef["u"] * (xv.u.values - bv.u.values.mean()), rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError, match="background_frame"):
        glm.predict_contributions(x, output_per_reference=True)
    same = glm.predict_contributions(x, background_frame=None)
    for u, v in zip(same.vecs, glm.predict_contributions(x).vecs):
        assert torch.equal(u.data, v.data)


def test_cluster_op_gathers_background_and_offsets_rows(model, data):
    """op_predict on rank 1 of 2, with a stand-in communicator whose gather
    returns both ranks' (identical) shards: the background is the gathered
    frame and RowIdx counts from the rows of the lower rank."""
    from types import SimpleNamespace

    from h2omx.runtime.ops import op_predict

    _, x, b = data
    comm = SimpleNamespace(world_size=2, all_gather_cat=lambda t, dim=0: torch.cat([t, t], dim=dim),
                           all_reduce_numpy=lambda a, op="sum": a * 2)
    cl = SimpleNamespace(world_size=2, rank=1, comm=comm)
    try:
        DKV.put("op_model", model)
        DKV.put("op_x", x)
        DKV.put("op_b", b)
        out = op_predict(cl, "op_model", "op_x", "op_pairs", kind="contributions", background_frame="op_b",
                         output_per_reference=True)
        got = DKV.get("op_pairs")
        assert got.nrows == 3 * 10 and out["rows"] == 60
        np.testing.assert_array_equal(got.vec("RowIdx").data.numpy(), 3 + np.repeat(np.arange(3), 10))
        np.testing.assert_array_equal(got.vec("BackgroundRowIdx").data.numpy(), np.tile(np.arange(10), 3))
        one = predict_contributions(model, x, background_frame=b, output_per_reference=True)
        for c in "pqrs":
            np.testing.assert_array_equal(got.vec(c).data.numpy().reshape(3, 2, 5)[:, 0],
                                          one.vec(c).data.numpy().reshape(3, 5))
        op_predict(cl, "op_model", "op_x", "op_avg", kind="contributions", background_frame="op_b")
        avg = predict_contributions(model, x, background_frame=b)
        for u, v in zip(DKV.get("op_avg").vecs, avg.vecs):
            np.testing.assert_allclose(u.data.numpy(), v.data.numpy(), atol=1e-6)
        with pytest.raises(ValueError, match="background_frame"):
            op_predict(cl, "op_model", "op_x", "op_bad", kind="contributions", output_per_reference=True)
    finally:
        DKV.clear()


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
    fr = Frame.from_pandas(_data(600, seed=4), key="bgtrain.hex")
    DKV.put("bgtrain.hex", fr)
    DKV.put("bgx.hex", Frame(fr.rows(torch.arange(0, 9)).vecs, key="bgx.hex"))
    DKV.put("bgb.hex", Frame(fr.rows(torch.arange(20, 24)).vecs, key="bgb.hex"))
    m = conn.train("gbm", "bgtrain.hex", y="y", ntrees=4, max_depth=3, seed=1)
    mid = m["model_id"]["name"]
    model = DKV.get(mid)
    # the client over HTTP: H2OApi.handle -> cluster op -> explain
    key = conn.predict_contributions(mid, "bgx.hex", background_frame="bgb.hex")
    got = DKV.get(key)
    assert got.names == ["p", "q", "r", "s", "BiasTerm"] and got.nrows == 9
    want = predict_contributions(model, DKV.get("bgx.hex"), background_frame=DKV.get("bgb.hex"))
    for u, v in zip(got.vecs, want.vecs):
        assert torch.equal(u.data, v.data)
    key = conn.predict_contributions(mid, "bgx.hex", background_frame="bgb.hex", output_per_reference=True)
    cols = conn.frame(key, rows=3)
    assert [c["label"] for c in cols["columns"]] == ["RowIdx", "BackgroundRowIdx", "p", "q", "r", "s", "BiasTerm"]
    assert cols["rows"] == 36
    assert DKV.get(conn.predict_contributions(mid, "bgx.hex")).names == ["p", "q", "r", "s", "BiasTerm"]
    # handle() itself: the forwarded parameters and the error answers
    base = f"/3/Predictions/models/{mid}/frames/bgx.hex"
    status, _, out = api.handle("POST", base, {"predict_contributions": "true", "background_frame": "bgb.hex",
                                               "output_per_reference": "true", "predictions_frame": "bgpairs"})
    assert status == 200 and out["predictions_frame"]["name"] == "bgpairs" and DKV.get("bgpairs").nrows == 36
    status, _, err = api.handle("POST", base, {"predict_contributions": "true", "background_frame": "bgb.hex",
                                               "output_space": "true"})
    assert status >= 400 and "output_space" in err["msg"]
    status, _, err = api.handle("POST", base, {"predict_contributions": "true", "output_per_reference": "true"})
    assert status >= 400 and "background_frame" in err["msg"]
    status, _, err = api.handle("POST", base, {"predict_contributions": "true", "background_frame": "nope.hex"})
    assert status == 404
    with pytest.raises(H2OResponseError):
        conn.request(f"POST {base}", {"predict_contributions": True, "output_space": True})


