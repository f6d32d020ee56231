"""DeepSHAP, ``predict_contributions(frame, background_frame=...)`` of a Deep
Learning model, on CPU frames: against the float64 pair-by-pair oracle of
tests/deepshap_ref.py in both output forms, completeness against the model's
own margin, exact Shapley values on an additive net against a brute-force
enumeration scored by the model, exact zeros and ties, the refusals, the
ranked form and the REST round trip (tests/test_deepshap_gpu.py runs the HIP
kernels)."""
import itertools
import math

import numpy as np
import pytest
import torch

import deepshap_ref as DR
from h2omx.api.server import H2OApi
from h2omx.explain import predict_contributions, rank_contributions
from h2omx.frame import Frame
from h2omx.frame.frame import DKV
from h2omx.models import H2ODeepLearningEstimator, H2OKMeansEstimator
from h2omx.runtime.cluster import ClusterConfig, form_cluster

N_X, N_B = 9, 5
PRED = ["x0", "x1", "g", "x2", "x3"]


def _frames(kind, seed=0):
    df = DR.make_df(500 + N_X + N_B, seed, kind=kind)
    train = Frame.from_pandas(df.iloc[:500].reset_index(drop=True))
    x = Frame.from_pandas(df.iloc[500: 500 + N_X].drop(columns="y").reset_index(drop=True))
    b = Frame.from_pandas(df.iloc[500 + N_X:].drop(columns="y").reset_index(drop=True))
    return train, x, b


CASES = [(a, h, k) for a in DR.ACTS for h, k in (((5,), "binomial"), ((5, 3), "regression"))]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}")
def case(request):
    act, hidden, kind = request.param
    train, x, b = _frames(kind)
    m = DR.fit(train, act, hidden)
    xs, bs = DR.design_rows(m, x), DR.design_rows(m, b)
    assert xs.shape == (N_X, 7) and m.design.spec[2:5] == [("g", 0), ("g", 1), ("g", 2)]
    assert DR.min_gap(m, xs, bs) >= 1e-6          # the oracle's naive quotient keeps >= 9 digits
    Zx, _ = DR._forward(m, xs)
    assert all((z > 0).any() and (z < 0).any() for z in Zx)
    phi, mx, mb = DR.oracle(m, xs, bs)
    phi.setflags(write=False)
    return dict(m=m, x=x, b=b, phi=phi, mx=mx, mb=mb)


def _tol(ref):
    # float64 arithmetic, results stored as float32 (2^-24 relative)
    return 1e-6 * max(1.0, float(np.abs(ref).max()))


def test_matches_oracle_in_both_forms(case):
    m, phi = case["m"], case["phi"]
    avg = predict_contributions(m, case["x"], background_frame=case["b"])
    assert avg.names == PRED + ["BiasTerm"] and avg.nrows == N_X
    np.testing.assert_allclose(DR.stack(avg, PRED).T, phi.mean(1), atol=_tol(phi))
    np.testing.assert_allclose(avg.vec("BiasTerm").data.numpy(), np.full(N_X, case["mb"].mean()), atol=_tol(case["mb"]))
    per = m.predict_contributions(case["x"], background_frame=case["b"], output_per_reference=True)
    assert per.names == ["RowIdx", "BackgroundRowIdx"] + PRED + ["BiasTerm"] and per.nrows == N_X * N_B
    np.testing.assert_array_equal(per.vec("RowIdx").data.numpy(), np.repeat(np.arange(N_X), N_B))
    np.testing.assert_array_equal(per.vec("BackgroundRowIdx").data.numpy(), np.tile(np.arange(N_B), N_X))
    np.testing.assert_allclose(DR.stack(per, PRED).T.reshape(N_X, N_B, -1), phi, atol=_tol(phi))
    np.testing.assert_allclose(per.vec("BiasTerm").data.numpy(), np.tile(case["mb"], N_X), atol=_tol(case["mb"]))


def _margin(m, frame):
    P = m.predict_raw(m.adapt_frame(frame)).double()
    return (torch.log(P[1]) - torch.log(P[0])).numpy() if P.shape[0] == 2 else P[0].numpy()


def test_completeness_against_the_models_margin(case):
    m = case["m"]
    mx = _margin(m, case["x"])
    tol = 5e-4 * max(1.0, float(np.abs(mx).max()))        # the model scores in float32
    avg = predict_contributions(m, case["x"], background_frame=case["b"])
    np.testing.assert_allclose(DR.stack(avg, avg.names).sum(0), mx, atol=tol)
    per = predict_contributions(m, case["x"], background_frame=case["b"], output_per_reference=True)
    np.testing.assert_allclose(DR.stack(per, per.names[2:]).sum(0), np.repeat(mx, N_B), atol=tol)
    np.testing.assert_allclose(per.vec("BiasTerm").data.numpy(), np.tile(_margin(m, case["b"]), N_X), atol=tol)


@pytest.mark.parametrize("act", DR.ACTS)
def test_exact_shapley_on_an_additive_net(act):
    """Every hidden unit reads one predictor, so the model is a sum of
    one-variable functions: the rescale rule is then exactly the Shapley value
    of the hybrid-row game, enumerated here over all 16 coalitions and scored
    by the model itself."""
    df = DR.make_df(520, 3, enum=False)
    m = DR.fit(Frame.from_pandas(df.iloc[:500].reset_index(drop=True)), act, (6,))
    W0 = m.net.W(0)
    keep = torch.zeros_like(W0)
    for u in range(6):
        keep[u, u % 4] = 1.0
    W0.mul_(keep)
    raw = df[DR.NUM].to_numpy(np.float32)
    X, B = raw[500:504], raw[510:513]
    assert not np.isnan(X).any() and not np.isnan(B).any()
    masks = list(itertools.product((False, True), repeat=4))
    rows = np.stack([np.where(T, x, b) for x in X for b in B for T in masks])
    v = _margin(m, Frame.from_numpy(rows, names=DR.NUM)).reshape(4, 3, 16)
    idx = {T: i for i, T in enumerate(masks)}
    phi = np.zeros((4, 3, 4))
    for j in range(4):
        for T in masks:
            if not T[j]:
                k = sum(T)
                Tj = tuple(True if i == j else t for i, t in enumerate(T))
                phi[:, :, j] += math.factorial(k) * math.factorial(3 - k) / 24 * (v[:, :, idx[Tj]] - v[:, :, idx[T]])
    per = predict_contributions(m, Frame.from_numpy(X, names=DR.NUM),
                                background_frame=Frame.from_numpy(B, names=DR.NUM), output_per_reference=True)
    assert np.abs(phi).max() > 0.05
    np.testing.assert_allclose(DR.stack(per, DR.NUM).T.reshape(4, 3, 4), phi, atol=1e-4 * max(1.0, np.abs(v).max()))


def test_a_row_explained_against_itself_is_exactly_zero(case):
    m, b = case["m"], case["b"]
    per = predict_contributions(m, b, background_frame=b, output_per_reference=True)
    got = DR.stack(per, PRED).T.reshape(N_B, N_B, -1)
    assert np.isfinite(got).all()
    for r in range(N_B):
        assert np.all(got[r, r] == 0.0)
    assert np.abs(got).max() > 0


@pytest.mark.parametrize("act", DR.ACTS)
def test_a_unit_that_ties_for_every_pair(act):
    """A hidden unit with an all-zero weight row has zx == zb (its bias) for
    every pair: the multiplier is the derivative there, finite, and the unit
    still passes nothing down."""
    train, x, b = _frames("regression", seed=5)
    m = DR.fit(train, act, (5, 3))
    m.net.W(0)[2].zero_()
    m.net.W(1)[1].zero_()
    m.net.b(1)[1] = -0.25
    xs, bs = DR.design_rows(m, x), DR.design_rows(m, b)
    assert DR.min_gap(m, xs, bs) >= 1e-6
    phi, _, _ = DR.oracle(m, xs, bs)
    per = predict_contributions(m, x, background_frame=b, output_per_reference=True)
    got = DR.stack(per, PRED).T.reshape(N_X, N_B, -1)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, phi, atol=_tol(phi))


def test_a_net_without_hidden_layers_is_linear_shap():
    train, x, b = _frames("regression", seed=2)
    m = DR.fit(train, "Tanh", ())
    phi, _, _ = DR.oracle(m, DR.design_rows(m, x), DR.design_rows(m, b))
    per = predict_contributions(m, x, background_frame=b, output_per_reference=True)
    np.testing.assert_allclose(DR.stack(per, PRED).T.reshape(N_X, N_B, -1), phi, atol=_tol(phi))


def test_refusals():
    train, x, b = _frames("binomial")
    m = DR.fit(train, "Tanh", (4,))
    with pytest.raises(ValueError, match="needs a background_frame"):
        predict_contributions(m, x)
    with pytest.raises(ValueError, match="needs a background_frame"):
        predict_contributions(m, x, output_per_reference=True)
    with pytest.raises(ValueError, match="no rows"):
        predict_contributions(m, x, background_frame=b.rows(torch.arange(0)))
    with pytest.raises(ValueError, match="output_format"):
        predict_contributions(m, x, background_frame=b, output_format="Wide")
    multi = DR.fit(_frames("multinomial")[0], "Tanh", (4,))
    with pytest.raises(ValueError, match="multinomial"):
        predict_contributions(multi, x, background_frame=b)
    maxout = DR.fit(train, "Maxout", (4,))
    with pytest.raises(ValueError, match="Maxout"):
        predict_contributions(maxout, x, background_frame=b)
    auto = H2ODeepLearningEstimator(hidden=[3], epochs=0.1, autoencoder=True, seed=1).train(
        x=PRED, training_frame=train)
    with pytest.raises(ValueError, match="autoencoder"):
        predict_contributions(auto, x, background_frame=b)
    off = DR.fit(_frames("regression")[0], "Tanh", (4,), offset_column="x3")
    with pytest.raises(ValueError, match="offset_column"):
        predict_contributions(off, x, background_frame=b)
    import h2omx.explain as ex

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ex, "_CPU_CONTRIB_LIMIT", 100)
        with pytest.raises(ValueError, match=rf"{N_X} rows against {N_B} background rows.*1440 bytes.*100 bytes"):
            predict_contributions(m, x, background_frame=b, output_per_reference=True)


def test_other_models_keep_their_error():
    train, x, b = _frames("regression")
    km = H2OKMeansEstimator(k=2, seed=1).train(x=DR.NUM, training_frame=train)
    with pytest.raises(NotImplementedError, match="predict_contributions is available for tree models, not kmeans"):
        predict_contributions(km, x, background_frame=b)


@pytest.mark.parametrize("kw", [dict(top_n=2), dict(bottom_n=3, compare_abs=True), dict(top_n=1, bottom_n=2),
                                dict(top_n=-1)])
def test_ranked_form_is_the_ranked_unsorted_frame(case, kw):
    m = case["m"]
    for per in (False, True):
        plain = predict_contributions(m, case["x"], background_frame=case["b"], output_per_reference=per)
        got = predict_contributions(m, case["x"], background_frame=case["b"], output_per_reference=per, **kw)
        want = rank_contributions(plain, kw.get("top_n"), kw.get("bottom_n"), kw.get("compare_abs", False),
                                  nlead=2 if per else 0)
        assert got.names == want.names and got.names != plain.names
        for u, v in zip(got.vecs, want.vecs):
            assert torch.equal(u.data, v.data), u.name
        assert got.vec(got.names[2 if per else 0]).domain == PRED


def test_rest_round_trip():
    train, x, b = _frames("binomial")
    m = DR.fit(train, "ExpRectifier", (5, 3))
    api = H2OApi(form_cluster(ClusterConfig(), device="cpu"))
    try:
        DKV.put("ds_model", m)
        DKV.put("ds_x.hex", Frame(x.vecs, key="ds_x.hex"))
        DKV.put("ds_b.hex", Frame(b.vecs, key="ds_b.hex"))
        base = "/3/Predictions/models/ds_model/frames/ds_x.hex"
        status, _, out = api.handle("POST", base, {"predict_contributions": "true", "background_frame": "ds_b.hex",
                                                   "predictions_frame": "ds_avg"})
        assert status == 200 and out["predictions_frame"]["name"] == "ds_avg"
        want = predict_contributions(m, x, background_frame=b)
        got = DKV.get("ds_avg")
        assert got.names == PRED + ["BiasTerm"]
        for u, v in zip(got.vecs, want.vecs):
            assert torch.equal(u.data, v.data)
        status, _, out = api.handle("POST", base, {"predict_contributions": "true", "background_frame": "ds_b.hex",
                                                   "output_per_reference": "true", "top_n": "2",
                                                   "predictions_frame": "ds_top"})
        assert status == 200 and DKV.get("ds_top").nrows == N_X * N_B
        assert DKV.get("ds_top").names[:3] == ["RowIdx", "BackgroundRowIdx", "top_feature_1"]
        status, _, err = api.handle("POST", base, {"predict_contributions": "true"})
        assert status >= 400 and "background_frame" in err["msg"]
    finally:
        DKV.clear()
