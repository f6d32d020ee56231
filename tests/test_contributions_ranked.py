"""Ranked contributions, ``predict_contributions(frame, top_n=, bottom_n=,
compare_abs=)``, on the CPU: ``_rank_numpy`` against a brute-force ``sorted``
oracle on hand-made ties, ``_rank_spec`` on every row of its table, the public
call in the three tree SHAP forms and for a GLM against ``_rank_numpy`` of the
unsorted call's own output, and the cluster op / REST / client round trip
(tests/test_contributions_ranked_gpu.py runs the HIP kernel).  Ranking moves
floats and computes none, so every comparison is exact."""
import socket

import numpy as np
import pandas as pd
import pytest
import torch

from h2omx.api.server import H2OApi, serve
from h2omx.client import H2OConnection
from h2omx.explain import _rank_numpy, _rank_spec, predict_contributions
from h2omx.frame import Frame
from h2omx.frame.frame import DKV, ENUM
from h2omx.models import (H2OGeneralizedLinearEstimator, H2OGradientBoostingEstimator,
                          H2ORandomForestEstimator)
from h2omx.runtime.cluster import ClusterConfig, form_cluster


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def brute_rank(phi, kt, kb, compare_abs):
    """(idx, val) [kt + kb][n] by Python's ``sorted`` on (-key, f) and (key, f)."""
    F, n = phi.shape
    idx = np.empty((kt + kb, n), np.int32)
    for r in range(n):
        key = [abs(float(x)) if compare_abs else float(x) for x in phi[:, r]]
        desc = sorted(range(F), key=lambda f: (-key[f], f))
        asc = sorted(range(F), key=lambda f: (key[f], f))
        idx[:, r] = desc[:kt] + asc[:kb]
    return idx, np.take_along_axis(phi, idx, 0)


def all_specs(F):
    """Every (kt, kb) the resolution table can produce for F columns."""
    return ([(k, 0) for k in range(1, F + 1)] + [(0, k) for k in range(1, F + 1)]
            + [(t, b) for t in range(1, F) for b in range(1, F) if t + b < F])


# columns of HAND are rows of the scored frame; phi is [F][n]
HAND = np.array([
    [1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5],            # all equal
    [0.0, 0.0, 0.0, -0.0, 0.0, 0.0, 0.0],           # zeros, one of them negative
    [2.0, -2.0, 0.5, -0.5, 0.5, 3.0, -3.0],         # +a and -a: ties under compare_abs
    [1.0, 1.0, 2.0, 2.0, 0.0, 0.0, 1.0],            # ascending is not descending reversed
    [0.3, -1.2, 5.0, -7.0, 0.01, 2.0, -0.4],        # all distinct
    [-0.0, 0.0, -1.0, 1.0, -0.0, 0.0, 1.0],         # signed zeros among ties
], np.float32).T.copy()


@pytest.mark.parametrize("F", [1, 2, 7])
@pytest.mark.parametrize("compare_abs", [False, True])
def test_rank_numpy_matches_bruteforce(F, compare_abs):
    phi = np.ascontiguousarray(HAND[:F])
    assert np.signbit(HAND[3, 1]) and not np.signbit(HAND[2, 1])
    for kt, kb in all_specs(F):
        idx, val = _rank_numpy(phi, kt, kb, compare_abs)
        ridx, rval = brute_rank(phi, kt, kb, compare_abs)
        assert idx.dtype == np.int32 and val.dtype == np.float32 and idx.shape == (kt + kb, phi.shape[1])
        assert np.array_equal(idx, ridx), (kt, kb)
        assert np.array_equal(bits(val), bits(rval)), (kt, kb)      # bit for bit: a zero keeps its sign


def test_ascending_is_not_reversed_descending():
    idx, _ = _rank_numpy(HAND, 7, 0, False)
    asc, _ = _rank_numpy(HAND, 0, 7, False)
    assert list(idx[:, 3]) == [2, 3, 0, 1, 6, 4, 5] and list(asc[:, 3]) == [4, 5, 0, 1, 6, 2, 3]
    assert list(asc[:, 3]) != list(idx[::-1, 3])
    assert list(idx[:, 0]) == list(asc[:, 0]) == list(range(7))          # all equal: index order both ways
    assert list(idx[:, 1]) == list(asc[:, 1]) == list(range(7))          # -0.0 ties with +0.0
    top, _ = _rank_numpy(HAND, 2, 0, True)
    assert list(top[:, 2]) == [5, 6]                                     # |3.0| == |-3.0|: the lower index first


@pytest.mark.parametrize("top_n,bottom_n,F,want", [
    (0, 0, 7, (0, 0)), (None, None, 7, (0, 0)), (None, 0, 7, (0, 0)),
    (-1, 0, 7, (7, 0)), (-5, 3, 7, (7, 0)), (-1, -1, 7, (7, 0)), (2, -1, 7, (7, 0)), (-1, None, 7, (7, 0)),
    (0, -1, 7, (0, 7)), (None, -3, 7, (0, 7)),
    (3, 0, 7, (3, 0)), (3, None, 7, (3, 0)), (7, 0, 7, (7, 0)), (9, 0, 7, (7, 0)), (1, 0, 1, (1, 0)),
    (0, 2, 7, (0, 2)), (None, 2, 7, (0, 2)), (0, 100, 7, (0, 7)),
    (3, 4, 7, (7, 0)), (4, 4, 7, (7, 0)), (9, 1, 7, (7, 0)),            # t + b >= F
    (3, 3, 7, (3, 3)), (1, 5, 7, (1, 5)), (1, 1, 3, (1, 1)), (1, 1, 2, (2, 0)),
    (2.0, 3.0, 7, (2, 3)), (np.int64(2), np.float32(1.0), 7, (2, 1)),
])
def test_rank_spec_table(top_n, bottom_n, F, want):
    assert _rank_spec(top_n, bottom_n, F) == want


@pytest.mark.parametrize("top_n,bottom_n,name", [(1.5, 0, "top_n"), (0, 2.25, "bottom_n"), ("3", 0, "top_n"),
                                                  (None, "abc", "bottom_n"), (float("nan"), 0, "top_n"),
                                                  (True, 0, "top_n")])
def test_rank_spec_refuses_non_integers(top_n, bottom_n, name):
    with pytest.raises(ValueError, match=name):
        _rank_spec(top_n, bottom_n, 7)


# ---------------------------------------------------------------------------
# public call
# ---------------------------------------------------------------------------
COLS = ["a", "b", "c", "k", "e"]            # k is constant: never split, its contribution is exactly zero


def _data(n=300, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 3)).astype(np.float32)
    X[::17, 1] = np.nan
    X[5::29, 2] = np.nan
    e = rng.choice(["u", "v", "w", "x"], n)
    f = X[:, 0] - np.nan_to_num(X[:, 1]) * np.nan_to_num(X[:, 2]) + np.where(e == "w", 1.5, 0.0)
    df = pd.DataFrame(X, columns=list("abc"))
    df["k"] = np.float32(2.5)
    df["e"] = pd.Categorical(e)
    df["yreg"] = (f + 0.1 * rng.normal(size=n)).astype(np.float32)
    df["ycls"] = pd.Categorical(np.where(f + 0.3 * rng.normal(size=n) > 0, "p", "q"))
    return df


@pytest.fixture(scope="module")
def frames():
    df = _data()
    return Frame.from_pandas(df), Frame.from_pandas(df.iloc[40:77].reset_index(drop=True)), \
        Frame.from_pandas(df.iloc[200:211].reset_index(drop=True))


@pytest.fixture(scope="module", params=["gbm_regression", "drf_binomial"])
def model(request, frames):
    if request.param == "gbm_regression":
        return H2OGradientBoostingEstimator(ntrees=6, max_depth=3, seed=1).train(x=COLS, y="yreg",
                                                                                 training_frame=frames[0])
    return H2ORandomForestEstimator(ntrees=4, max_depth=4, seed=1).train(x=COLS, y="ycls", training_frame=frames[0])


REQUESTS = [
    # top_n, bottom_n, compare_abs -> (kt, kb) for F = 5
    (3, None, False, (3, 0)), (None, 2, False, (0, 2)), (2, 2, False, (2, 2)), (3, 2, False, (5, 0)),
    (-1, None, False, (5, 0)), (0, -1, False, (0, 5)), (100, 0, False, (5, 0)),
    (3, None, True, (3, 0)), (1, 3, True, (1, 3)), (-1, 0, True, (5, 0)),
]


def ranked_names(kt, kb, lead=()):
    names = list(lead)
    for side, k in (("top", kt), ("bottom", kb)):
        for i in range(1, k + 1):
            names += [f"{side}_feature_{i}", f"{side}_value_{i}"]
    return names + ["BiasTerm"]


def check_ranked(plain: Frame, ranked: Frame, kt, kb, compare_abs, names, nlead=0):
    """``ranked`` is the ranked form of the unsorted frame ``plain``: names,
    types, and per row exactly ``_rank_numpy`` of plain's own contributions."""
    lead = plain.names[:nlead]
    assert plain.names == lead + list(names) + ["BiasTerm"]
    assert ranked.names == ranked_names(kt, kb, lead)
    assert ranked.nrows == plain.nrows
    phi = torch.stack([plain.vec(c).data for c in names]).cpu().numpy()
    assert phi.dtype == np.float32
    idx, val = _rank_numpy(phi, kt, kb, compare_abs)
    for s in range(kt + kb):
        fv, vv = ranked.vecs[nlead + 2 * s], ranked.vecs[nlead + 2 * s + 1]
        assert fv.vtype == ENUM and list(fv.domain) == list(names) and vv.vtype == "real"
        assert np.array_equal(fv.data.cpu().numpy(), idx[s]), fv.name
        assert np.array_equal(bits(vv.data.cpu().numpy()), bits(val[s])), vv.name
    for c in lead + ["BiasTerm"]:
        assert torch.equal(ranked.vec(c).data, plain.vec(c).data), c
    return phi, idx, val


def test_path_dependent_ranked(model, frames):
    fr = frames[0]
    plain = predict_contributions(model, fr)
    assert bool((plain.vec("k").data == 0).all())                 # the zero ties are real
    for top_n, bottom_n, ca, (kt, kb) in REQUESTS:
        ranked = model.predict_contributions(fr, top_n=top_n, bottom_n=bottom_n, compare_abs=ca)
        phi, idx, val = check_ranked(plain, ranked, kt, kb, ca, COLS)
        if kt == 5 or kb == 5:                                    # all of them: a permutation of the row
            assert np.array_equal(np.sort(idx, 0), np.tile(np.arange(5, dtype=np.int32)[:, None], (1, fr.nrows)))
            assert np.array_equal(np.sort(val, 0), np.sort(phi, 0))


def test_output_format_and_unsorted_default(model, frames):
    fr = frames[1]
    plain = predict_contributions(model, fr)
    a = predict_contributions(model, fr, top_n=2, bottom_n=1, output_format="Original")
    b = predict_contributions(model, fr, top_n=2, bottom_n=1, output_format="compact")
    assert a.names == b.names and all(torch.equal(u.data, v.data) for u, v in zip(a.vecs, b.vecs))
    with pytest.raises(ValueError, match="'x'"):
        predict_contributions(model, fr, top_n=2, output_format="x")
    with pytest.raises(ValueError, match="'x'"):
        predict_contributions(model, fr, output_format="x")
    with pytest.raises(ValueError, match="top_n"):
        predict_contributions(model, fr, top_n=1.5)
    for kw in (dict(top_n=0, bottom_n=0), dict(top_n=None, bottom_n=None, compare_abs=True),
               dict(output_format="Compact")):
        same = model.predict_contributions(fr, **kw)
        assert same.names == plain.names == COLS + ["BiasTerm"]
        assert all(torch.equal(u.data, v.data) for u, v in zip(same.vecs, plain.vecs))


def test_background_forms_ranked(model, frames):
    _, x, b = frames
    n, nb = x.nrows, b.nrows
    avg = predict_contributions(model, x, background_frame=b)
    per = predict_contributions(model, x, background_frame=b, output_per_reference=True)
    assert per.nrows == n * nb
    for top_n, bottom_n, ca, (kt, kb) in REQUESTS[:4] + REQUESTS[7:9]:
        kw = dict(top_n=top_n, bottom_n=bottom_n, compare_abs=ca)
        check_ranked(avg, predict_contributions(model, x, background_frame=b, **kw), kt, kb, ca, COLS)
        got = model.predict_contributions(x, background_frame=b, output_per_reference=True, **kw)
        check_ranked(per, got, kt, kb, ca, COLS, nlead=2)
        assert got.nrows == n * nb
        np.testing.assert_array_equal(got.vec("RowIdx").data.numpy(), np.repeat(np.arange(n), nb))
        np.testing.assert_array_equal(got.vec("BackgroundRowIdx").data.numpy(), np.tile(np.arange(nb), n))


def test_per_reference_size_check_counts_the_ranked_result(model, frames, monkeypatch):
    import h2omx.explain as ex

    _, x, b = frames
    n, nb = x.nrows, b.nrows
    unranked = 4 * n * nb * (5 + 3)
    monkeypatch.setattr(ex, "_CPU_CONTRIB_LIMIT", unranked)
    predict_contributions(model, x, background_frame=b, output_per_reference=True)       # fits exactly
    with pytest.raises(ValueError, match=rf"{n} rows against {nb} background rows needs "
                                         rf"{unranked + 8 * 3 * n * nb} bytes.*limit is {unranked} bytes"):
        predict_contributions(model, x, background_frame=b, output_per_reference=True, top_n=1, bottom_n=2)


def test_glm_binomial_ranked(frames):
    fr, x, b = frames
    glm = H2OGeneralizedLinearEstimator(family="binomial", lambda_=0.0).train(x=COLS, y="ycls", training_frame=fr)
    plain = glm.predict_contributions(fr)
    names = plain.names[:-1]
    F = len(names)
    assert "e" in names and F >= 4                       # the one-hot columns of e are folded back
    for top_n, bottom_n, ca in [(2, None, False), (None, 2, False), (1, 1, False), (-1, None, True), (0, -1, False)]:
        kt, kb = _rank_spec(top_n, bottom_n, F)
        check_ranked(plain, glm.predict_contributions(fr, top_n=top_n, bottom_n=bottom_n, compare_abs=ca), kt, kb,
                     ca, names)
    per = glm.predict_contributions(x, background_frame=b, output_per_reference=True)
    got = glm.predict_contributions(x, background_frame=b, output_per_reference=True, top_n=1, bottom_n=1)
    check_ranked(per, got, 1, 1, False, names, nlead=2)
    avg = glm.predict_contributions(x, background_frame=b)
    check_ranked(avg, glm.predict_contributions(x, background_frame=b, top_n=2, compare_abs=True), 2, 0, True, names)
    with pytest.raises(ValueError, match="'x'"):
        glm.predict_contributions(fr, top_n=1, output_format="x")
    with pytest.raises(ValueError, match="bottom_n"):
        glm.predict_contributions(fr, bottom_n=0.5)
    same = glm.predict_contributions(fr, top_n=0, bottom_n=0, output_format="Compact")
    assert all(torch.equal(u.data, v.data) for u, v in zip(same.vecs, plain.vecs))


# ---------------------------------------------------------------------------
# cluster op, REST, client
# ---------------------------------------------------------------------------
def test_cluster_op_passes_and_refuses_the_keywords(model, frames):
    from types import SimpleNamespace

    from h2omx.runtime.ops import op_predict

    _, x, b = frames
    cl = SimpleNamespace(world_size=1, rank=0, comm=None)
    try:
        DKV.put("rk_model", model)
        DKV.put("rk_x", x)
        DKV.put("rk_b", b)
        op_predict(cl, "rk_model", "rk_x", "rk_top", kind="contributions", top_n=2, bottom_n=1, compare_abs=True)
        check_ranked(predict_contributions(model, x), DKV.get("rk_top"), 2, 1, True, COLS)
        op_predict(cl, "rk_model", "rk_x", "rk_pairs", kind="contributions", background_frame="rk_b",
                   output_per_reference=True, bottom_n=-1, output_format="Compact")
        check_ranked(predict_contributions(model, x, background_frame=b, output_per_reference=True),
                     DKV.get("rk_pairs"), 0, 5, False, COLS, nlead=2)
        for kw in (dict(top_n=2), dict(bottom_n=-1), dict(compare_abs=True), dict(output_format="Original")):
            with pytest.raises(ValueError, match="belong to predict_contributions"):
                op_predict(cl, "rk_model", "rk_x", "rk_bad", kind="predict", **kw)
        with pytest.raises(ValueError, match="'x'"):
            op_predict(cl, "rk_model", "rk_x", "rk_bad", kind="contributions", top_n=1, output_format="x")
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
    df = _data(300, seed=4).drop(columns="ycls")
    fr = Frame.from_pandas(df, key="rktrain.hex")
    DKV.put("rktrain.hex", fr)
    DKV.put("rkx.hex", Frame(fr.rows(torch.arange(0, 9)).vecs, key="rkx.hex"))
    DKV.put("rkb.hex", Frame(fr.rows(torch.arange(20, 24)).vecs, key="rkb.hex"))
    m = conn.train("gbm", "rktrain.hex", y="yreg", ntrees=4, max_depth=3, seed=1)
    mid = m["model_id"]["name"]
    model = DKV.get(mid)
    assert model.x == COLS
    x, b = DKV.get("rkx.hex"), DKV.get("rkb.hex")
    # the client over HTTP: H2OApi.handle -> cluster op -> explain
    got = DKV.get(conn.predict_contributions(mid, "rkx.hex", top_n=2, bottom_n=2))
    check_ranked(predict_contributions(model, x), got, 2, 2, False, COLS)
    got = DKV.get(conn.predict_contributions(mid, "rkx.hex", top_n=-1, compare_abs=True, output_format="Compact"))
    check_ranked(predict_contributions(model, x), got, 5, 0, True, COLS)
    key = conn.predict_contributions(mid, "rkx.hex", background_frame="rkb.hex", output_per_reference=True, bottom_n=1)
    check_ranked(predict_contributions(model, x, background_frame=b, output_per_reference=True), DKV.get(key), 0, 1,
                 False, COLS, nlead=2)
    cols = conn.frame(key, rows=3)
    assert [c["label"] for c in cols["columns"]] == ["RowIdx", "BackgroundRowIdx", "bottom_feature_1",
                                                    "bottom_value_1", "BiasTerm"]
    assert cols["rows"] == 36
    assert DKV.get(conn.predict_contributions(mid, "rkx.hex")).names == COLS + ["BiasTerm"]
    # handle() itself: the forwarded parameters and the error answers
    base = f"/3/Predictions/models/{mid}/frames/rkx.hex"
    status, _, out = api.handle("POST", base, {"predict_contributions": "true", "top_n": "1", "bottom_n": "0",
                                               "compare_abs": "true", "predictions_frame": "rktop",
                                               "predict_contributions_output_format": "Original"})
    assert status == 200 and out["predictions_frame"]["name"] == "rktop"
    check_ranked(predict_contributions(model, x), DKV.get("rktop"), 1, 0, True, COLS)
    for name in ("top_n", "bottom_n"):
        for bad in ("abc", "1.5"):
            status, _, err = api.handle("POST", base, {"predict_contributions": "true", name: bad})
            assert status == 400 and name in err["msg"], err
    status, _, err = api.handle("POST", base, {"predict_contributions": "true", "top_n": "1",
                                               "predict_contributions_output_format": "x"})
    assert status >= 400 and "'x'" in err["msg"]
    for kw in ({"top_n": "2"}, {"bottom_n": "-1"}, {"compare_abs": "true"},
               {"predict_contributions_output_format": "Compact"}):
        status, _, err = api.handle("POST", base, dict(kw))                 # a plain predict
        assert status >= 400 and "predict_contributions" in err["msg"], err
        status, _, err = api.handle("POST", base, dict(kw, leaf_node_assignment="true"))
        assert status >= 400 and "predict_contributions" in err["msg"], err
    status, _, err = api.handle("POST", base, {"predict_contributions": "true", "top_n": "2", "output_space": "true"})
    assert status >= 400 and "output_space" in err["msg"]
    status, _, out = api.handle("POST", f"/4/Predictions/models/{mid}/frames/rkx.hex",
                                {"predict_contributions": "true", "top_n": "2", "predictions_frame": "rkjob"})
    assert status == 200
    conn.wait_job(out["job"])
    check_ranked(predict_contributions(model, x), DKV.get("rkjob"), 2, 0, False, COLS)
